"""Generate tests/golden/ref_nanoflann_live.npz: the answers of the REFERENCE's own nanoflann (oracle/_ref, built from the reference
tree by oracle/Makefile -- data only, no reference source) that tests/test_oracle.py and tests/test_reference_pins.py hold the oracle
to, so that those tests need no reference tree where they run:

  knn_*     PointCloudKdtree (pcl_adaptor.hpp) 5-NN of 1 000 queries in a 30 000-point cloud (numpy default_rng(6), as the test draws it)
  radius_*  PointCloudKdtree::radiusSearch (r = 0.75 m) of the first 32 queries of ref_nanoflann_more.npz in its cloud, in the order
            the tree returns them: radius_idx / radius_d2 concatenated, radius_counts per query
  loam_*    the LOAM restatement searching through the reference's tree (oracle.use_reference_nanoflann): the refined pose and the
            convergence flag for the cloud of test_loam_oracle_on_reference_nanoflann
Run from the repo root where the reference tree (or a prebuilt oracle/_ref) is available:  python scripts/make_golden_ref_live.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import oracle  # noqa: E402
from simpleslam_amd import synth  # noqa: E402

G = os.path.join(ROOT, "tests", "golden")
oracle.build()
assert oracle.ref_available(), "oracle/_ref could not be built: no reference tree"
# ---- 5-NN ----
rng = np.random.default_rng(6)
pts = rng.uniform(-20, 20, (30000, 4)).astype(np.float32)
q = rng.uniform(-20, 20, (1000, 4)).astype(np.float32)
knn_idx, knn_d2 = oracle.ref_knn(pts, q, 5)
# ---- radius search ----
more = np.load(os.path.join(G, "ref_nanoflann_more.npz"))
r_idx, r_d2, r_cnt = [], [], []
for qq in more["knn_queries"][:32, :3].astype(np.float64):
    i, d = oracle.ref_radius(more["knn_points"], qq, 0.75)
    r_idx.append(np.asarray(i, np.int64)); r_d2.append(np.asarray(d, np.float64)); r_cnt.append(len(i))
print("radius search: sizes", min(r_cnt), "...", max(r_cnt))
# ---- LOAM through the reference's tree ----
world, m = synth.make_map(50_000, seed=77)
scan, T = synth.make_scan(world, 0, seed=77, beams=16, azimuths=512)
T0 = synth.perturb(T, 77)
prm = oracle.loam_params(iters=6, early_exit=0, threads=4)
try:
    oracle.use_reference_nanoflann(True)
    pose, conv, _ = oracle.loam_scan2map(scan, m, T0, prm)
finally:
    oracle.use_reference_nanoflann(False)
np.savez_compressed(os.path.join(G, "ref_nanoflann_live.npz"), knn_idx=knn_idx, knn_d2=knn_d2,
                    radius_idx=np.concatenate(r_idx), radius_d2=np.concatenate(r_d2), radius_counts=np.array(r_cnt, np.int64),
                    loam_pose=pose, loam_converged=np.array(int(conv), np.int64))
print("written")
