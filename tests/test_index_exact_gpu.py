"""Every kernel variant of the index build (csrc/grid_index.hip) against an exact cell table: host/index_check drives pcr::GridIndex through its
cases on the device -- each asserts the plan it ran (GridIndex::last_plan: what build() enqueued) before it compares the header, cell_start[0 .. n_cells]
and sorted[0 .. cell_start[n_cells]) with the counting sort of host/index_ref.hpp, exactly -- and prints which instantiations were reached by steps that
passed.  The program runs ONCE, in one process of its own (a device fault ends everything there, nothing is retried per case); the tests below read
what it printed.

Time limit of that run: measured on an MI355X, the whole program -- 52 cases, the four 2 M-point builds and their references included -- takes 1.4 s
(1 422 ms wall clock around the process, start of the HIP runtime included).  The limit is 120 s: the host side (generating and sorting 2 M-point
clouds) is single-threaded and a loaded or slower host may take several times as long; a hang is still ended within two minutes, and no test waits
for the limit when the program works."""
import os
import re
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "simpleslam_amd", "lib", "index_check")
TIMEOUT_S = 120

# (the program's own list: test_case_list_is_the_programs holds the two together)
CASES = [
    "one_level/n0", "one_level/n1", "one_level/n255", "one_level/n256", "one_level/n257", "one_level/one_cell", "one_level/scan_tile_boundary",
    "one_level/non_finite", "one_level/all_non_finite", "fresh/n0", "fresh/n1", "fresh/n255", "fresh/n256", "fresh/n257", "fresh/n2047",
    "fresh/n2048", "fresh/n2049", "fresh/n5000_partial_chunk", "fresh/non_finite", "fresh/all_non_finite", "fresh/stride4_vec", "fresh/stride8_vec",
    "fresh/stride3", "fresh/stride5", "fresh/stride4_one_float_in", "walk/vec", "walk/not_vec", "dense_coherent/walk", "room/exactly_full",
    "room/one_too_many", "stale/six_faces", "overflow/one_cell_too_many", "clamp/six_faces", "sparse/rings", "sparse/shuffled",
    "sparse/coherent_rings", "sparse/coherent_shuffled", "sparse/cut_clusters", "sparse/cut_coherent_clusters", "sparse/not_split", "pcl/leaf_0.1",
    "pcl/leaf_0.5", "shifted/cell_1", "shifted/cell_0.3", "filtered/bin_pass", "filtered/tail_per8", "filtered/tail_per16", "filtered/keep_2m",
    "filtered/keep_2m_dense", "twin/preset", "unrelated/hints", "unrelated/no_hints",
]


@pytest.fixture(scope="module")
def run(gpu):
    assert os.path.exists(EXE), "index_check not built (run __graft_entry__.build())"
    out = subprocess.run([EXE], capture_output=True, text=True, timeout=TIMEOUT_S)
    verdict = dict(re.findall(r"^case (\S+) (PASS|FAIL)$", out.stdout, re.M))
    cov = re.search(r"^coverage bin=(\S*) tile=(\S*) bins=\d+/\d+ tiles=\d+/\d+ place_vec=(\d) place_not_vec=(\d) keep=\d keep_vec=(\d) keep_not_vec=(\d) one_level=(\d)$", out.stdout, re.M)
    return dict(rc=out.returncode, out=out.stdout, err=out.stderr, verdict=verdict, cov=cov)


def _about(run, name):
    """the lines the program printed for one case"""
    m = re.search(r"^case %s\n(.*?)^case %s (PASS|FAIL)$" % (re.escape(name), re.escape(name)), run["out"], re.M | re.S)
    return m.group(1)[-6000:] if m else run["out"][-3000:] + run["err"][-2000:]


def test_case_list_is_the_programs():
    assert os.path.exists(EXE), "index_check not built (run __graft_entry__.build())"
    out = subprocess.run([EXE, "--list"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.split() == CASES


def test_no_hip_error(run):
    assert "HIP ERROR" not in run["out"] and run["rc"] in (0, 1), run["out"][-3000:] + run["err"][-2000:]


@pytest.mark.parametrize("name", CASES)
def test_case(run, name):
    assert run["verdict"].get(name) == "PASS", _about(run, name)


def test_every_variant_was_reached_by_a_passing_case(run):
    cov = run["cov"]
    assert cov is not None, run["out"][-3000:]
    assert cov.group(1) == "0,1,2,3,4,5,6,7", "bin variants reached: " + cov.group(1)
    assert cov.group(2) == "0,1,2,3,4,5,6,7,8,9", "tile variants reached: " + cov.group(2)
    assert (cov.group(3), cov.group(4)) == ("1", "1"), "grid_place_kernel<true> / <false>"
    assert (cov.group(5), cov.group(6)) == ("1", "1"), "grid_keep_kernel<true> / <false>"
    assert cov.group(7) == "1", "the one-level path"


def test_program_verdict(run):
    assert run["rc"] == 0, run["out"][-3000:] + run["err"][-2000:]
    assert run["out"].strip().splitlines()[-1] == "index_check ok: %d cases" % len(CASES)
