"""An asymmetric version of the synthetic city for global relocalisation tests.

synth.make_map builds a square grid of identical buildings: the scene has 4-fold rotational symmetry, and no place-recognition
method can tell mirrored places apart.  asymmetric_world drops a few buildings at asymmetric grid positions (dataclasses.replace on
world.boxes) and deletes their wall points from the map.  make_scan then raycasts against the remaining boxes; the ground under a
dropped footprint stays a hole in both the map and the scans (synth's ground test knows only the grid), so map and scans agree.

drive_poses lays key frames every `step` metres along a multi-leg drive through the streets; query_poses puts scans off that line
with arbitrary headings."""
import dataclasses
import math

import numpy as np

from simpleslam_amd import synth

DROPPED = ((0, 1), (1, 2), (3, 1))      # (i, j): the building whose footprint starts at (i, j) * PITCH + 10 m; no rotation of the square maps one onto another


def asymmetric_world(n_points, seed=0, spacing=0.5, dropped=DROPPED):
    """-> (world, map): make_map's world without the `dropped` buildings and the map without their walls (DROPPED, the drive and the
    queries are laid out for the 4 x 4 blocks of 300 000 points at 0.5 m or 1.4 M at 0.2 m)"""
    world, m = synth.make_map(n_points, seed=seed, spacing=spacing)
    assert max(max(c) for c in dropped) < world.blocks, f"make_map gave {world.blocks} x {world.blocks} blocks, too few for {dropped}"
    idx = [i * world.blocks + j for i, j in dropped]
    gone = world.boxes[idx]
    keep_box = np.ones(len(world.boxes), bool)
    keep_box[idx] = False
    w = m[:, :2].astype(np.float64) + synth.map_origin(world.blocks)[:2]
    drop = np.zeros(len(m), bool)
    for x0, y0, x1, y1 in gone:
        drop |= (w[:, 0] > x0 - 0.1) & (w[:, 0] < x1 + 0.1) & (w[:, 1] > y0 - 0.1) & (w[:, 1] < y1 + 0.1)
    return dataclasses.replace(world, boxes=world.boxes[keep_box].copy()), np.ascontiguousarray(m[~drop])


def planar_pose(world, x, y, yaw_deg):
    """the sensor at world (x, y) SENSOR_Z m above the ground, heading yaw_deg, in the map frame"""
    a = math.radians(yaw_deg)
    T = np.eye(4)
    T[:2, :2] = [[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]]
    T[:3, 3] = np.array([x, y, synth.SENSOR_Z]) - synth.map_origin(world.blocks)
    return T


# the drive (world coordinates): along the street y = 100 m from x = 20 to 180 m, then up the street x = 150 m from y = 100 to 180 m
LEGS = (((20.0, 100.0), (180.0, 100.0)), ((150.0, 102.0), (150.0, 180.0)))


def drive_poses(world, step=2.0):
    out = []
    for (xa, ya), (xb, yb) in LEGS:
        n = int(math.floor(math.hypot(xb - xa, yb - ya) / step)) + 1
        yaw = math.degrees(math.atan2(yb - ya, xb - xa))
        for k in range(n):
            t = k * step / math.hypot(xb - xa, yb - ya)
            out.append(planar_pose(world, xa + t * (xb - xa), ya + t * (yb - ya), yaw))
    return np.array(out)


# (x, y, heading): 0.3 - 1.5 m off the drive line, headings unrelated to the drive's
QUERIES = ((47.3, 100.9, 37.0), (91.0, 98.6, 143.0), (128.9, 100.4, -100.0), (171.2, 101.5, 61.0), (149.3, 125.1, -163.0), (150.8, 163.7, 12.0))


def query_poses(world):
    return np.array([planar_pose(world, x, y, yaw) for x, y, yaw in QUERIES])


def scan_at(world, T, seed, beams=64, azimuths=1024):
    """a scan taken at pose T (sensor frame)"""
    return synth.make_scan(world, 0, seed=seed, beams=beams, azimuths=azimuths, pose=T)[0]
