"""host/index_check compares every kernel variant of the index build with a plain counting sort (host/index_ref.hpp).  What of it runs without a
GPU: the reference itself against cell tables worked out by hand in the program's source (--self: faces, pad cells, negative coordinates, the shifted
and the pcl::VoxelGrid lattice, clamp, region mask, margins, overflow), the plan every case expects held to what plan_build() says for it (--plan:
no build is launched, the reference's header stands in for the device's), and the list of cases.  The device run is tests/test_index_exact_gpu.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "simpleslam_amd", "lib", "index_check")

# the groups of cases the program must have (the prefix of a case's name)
GROUPS = ["one_level", "fresh", "walk", "dense_coherent", "room", "stale", "overflow", "clamp", "sparse", "pcl", "shifted", "filtered", "twin", "unrelated"]


def _run(*args):
    assert os.path.exists(EXE), "index_check not built (run __graft_entry__.build())"
    return subprocess.run([EXE, *args], capture_output=True, text=True, timeout=300)


def test_reference_against_hand_worked_tables():
    out = _run("--self")
    assert out.returncode == 0, out.stdout[-4000:] + out.stderr[-2000:]
    assert out.stdout.strip() == "index_check --self ok"


def test_case_list_names_every_group():
    out = _run("--list")
    assert out.returncode == 0, out.stderr[-2000:]
    names = out.stdout.split()
    assert len(names) == len(set(names)) >= 50
    for g in GROUPS:
        assert any(n.startswith(g + "/") for n in names), f"no case of group {g}"
    for n in ["one_level/n0", "one_level/n257", "one_level/scan_tile_boundary", "one_level/all_non_finite", "fresh/n2047", "fresh/n2048", "fresh/n2049",
              "fresh/stride3", "fresh/stride4_one_float_in", "walk/vec", "walk/not_vec", "room/exactly_full", "room/one_too_many", "stale/six_faces",
              "sparse/cut_coherent_clusters", "pcl/leaf_0.1", "pcl/leaf_0.5", "filtered/keep_2m", "filtered/tail_per8", "twin/preset", "unrelated/no_hints"]:
        assert n in names, n


def test_expected_plans_are_what_the_planner_says():
    out = _run("--plan")
    assert out.returncode == 0, out.stdout[-6000:] + out.stderr[-2000:]
    assert out.stdout.strip().splitlines()[-1].startswith("index_check --plan ok")
    assert "MISMATCH" not in out.stdout
