#!/usr/bin/env python3
"""A map that follows the robot, and two robots' maps fused into one ("Re-framing and merging maps").

The world is a corridor 16 m long, 2 m wide and 1 m high, closed at both ends — more than three of the robot's boxes long.  The robot
carries an evidence map of 40 x 24 x 16 voxels of 0.125 m (5 m of corridor).  Every step it
  - calls tools.follow_map(map, position, margin): inside the margin that returns the very same map; near a side of the box it returns
    a new map with the robot's voxel in the middle, and everything still inside the box — evidence values, both planes — comes along.
    The margin along the corridor (14 voxels) exceeds the sensor's range (1.5 m = 12 voxels): the box's own edge is no frontier, so
    the unknown the robot plans towards has to lie inside the box;
  - scans all round with tools.depth_scan(..., into=map) — the ground truth is looked at through a window of the map's own box
    (tools.reframe_map of the world grid), because a scan goes into a map of the scanned grid's geometry;
  - plans in the moving box: tools.frontier_clusters(map) groups the frontier into openings, and the robot heads for the largest
    opening ahead of it, half a metre at a time.
It reaches the far end with a map that never grew, and that still holds what lies up to a box behind it.

Then two robots start at opposite ends and walk towards each other; their evidence maps — different boxes of one lattice — are fused
with tools.merge_maps into one map over the union box, on which tools.frontier_clusters runs: what is left to explore lies between
them.  Merging in either order gives the same bytes.

    python examples/rolling_map_sample.py [--steps 34] [--margin 14]
"""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from closed_loop_exploration_sample import all_round  # noqa: E402
from trajectory_optimization_amd import ops, synth  # noqa: E402
from trajectory_optimization_amd.tools import (depth_scan, evidence_map, follow_map, frontier_clusters, merge_maps, occupancy_grid,  # noqa: E402
                                                reframe_map)

LENGTH = 16.0
RES = 0.125
WORLD = dict(origin=(-0.5, -0.5, -0.5), dims=(136, 24, 16), resolution=RES)   # the whole corridor, half a metre around it
BOX = (40, 24, 16)                                                            # the robot's map: 5 m of it
SENSOR = dict(intrins=np.float32([[32.0, 0.0, 31.5], [0.0, 32.0, 23.5], [0.0, 0.0, 1.0]]), img_width=64, img_height=48, min_dist=0.05, max_dist=1.5)
START, STEP = (0.53, 0.97, 0.52), 0.5


def corridor_points(step=0.05):
    """The six faces of the box [0, LENGTH] x [0, 2] x [0, 1], sampled every `step` metres -> (N,3) f32."""
    x, y, z = (np.arange(int(round(n / step)) + 1) * step for n in (LENGTH, 2.0, 1.0))
    faces = []
    for v in (0.0, LENGTH):
        Y, Z = np.meshgrid(y, z, indexing="ij")
        faces.append(np.stack([np.full(Y.size, v), Y.ravel(), Z.ravel()], axis=1))
    for v in (0.0, 2.0):
        X, Z = np.meshgrid(x, z, indexing="ij")
        faces.append(np.stack([X.ravel(), np.full(X.size, v), Z.ravel()], axis=1))
    for v in (0.0, 1.0):
        X, Y = np.meshgrid(x, y, indexing="ij")
        faces.append(np.stack([X.ravel(), Y.ravel(), np.full(X.size, v)], axis=1))
    return np.concatenate(faces).astype(np.float32)


class Robot:
    """A position, a heading along the corridor (+1 or -1) and an evidence map that follows the position."""

    def __init__(self, world, position, heading, margin):
        self.world, self.position, self.heading, self.margin = world, np.float32(position), heading, margin
        self.map = reframe_map(evidence_map(world), centre=self.position, dims=BOX)   # an empty map around the start
        self.window = None       # the world seen through the map's box
        self.moves = 0

    def step(self):
        """follow, scan, plan, move -> (the clusters, whether the map moved)."""
        dev = self.map.device
        followed = follow_map(self.map, self.position, self.margin)
        moved = followed is not self.map
        if moved or self.window is None:
            self.map = followed
            self.moves += int(moved)
            self.window = reframe_map(self.world, shift=ops.lattice_offset(self.world, self.map), dims=BOX)
        poses, quats = all_round(self.position, synth.Q_OPTICAL)
        K = torch.from_numpy(SENSOR["intrins"])
        depth_scan(self.window, torch.from_numpy(poses).to(dev), torch.from_numpy(quats).to(dev), into=self.map, intrins=K,
                   **{k: v for k, v in SENSOR.items() if k != "intrins"})
        clusters = frontier_clusters(self.map, min_size=4)
        # head for the largest opening ahead (the rows come largest first), half a metre at a time along the corridor's axis
        ahead = [i for i in range(clusters.n) if self.heading * (float(clusters.centroids[i, 0]) - float(self.position[0])) > 0.25]
        # ... as long as the map calls the way free (the cones above and below the sensor's view leave openings everywhere)
        way = np.stack([self.position + np.float32([self.heading * d, 0.0, 0.0]) for d in (STEP, STEP + 0.25)])
        go = bool(ahead) and bool((self.map.log_odds(torch.from_numpy(way).to(dev))[1] == 1).all())
        if go:
            self.position = way[0]
        return clusters, moved, go

    def known(self):
        return int((self.map.dense() != ops.EVID_UNKNOWN).sum())


def make_world(device):
    world = occupancy_grid(device=device, **WORLD)
    world.insert(torch.from_numpy(corridor_points()).to(device))
    return world


def roll(steps=34, margin=(14, 2, 2), device="cuda:0", verbose=True):
    """One robot down the corridor -> (the robot, per-step records)."""
    world = make_world(torch.device(device))
    robot = Robot(world, START, +1, margin)
    records = []
    for t in range(steps):
        x = float(robot.position[0])
        before = robot.map
        clusters, moved, ahead = robot.step()
        if not moved and t > 0:
            assert robot.map is before, "inside the margin follow_map returns the identical map"
        rec = dict(step=t, x=x, origin_x=float(robot.map.origin[0]), moved=moved, known=robot.known(), clusters=clusters.n)
        records.append(rec)
        if verbose:
            print(f"step {t:2d}: at x = {x:5.2f}  box from x = {rec['origin_x']:6.3f}{'  (re-framed)' if moved else '':13s} "
                  f"{rec['known']:6d} known voxels, {clusters.n} frontier clusters of at least 4 voxels")
        if not ahead:
            if verbose:
                print("         no free way to an opening ahead: the far end is reached")
            break
    assert robot.moves >= 2, "the corridor is several boxes long: the map moved more than once"
    assert float(robot.position[0]) > LENGTH - 2.0, "the robot reached the far end"
    assert robot.map.dims == BOX
    # what the map knew before its last move and still holds came along: the wall voxels behind the robot are occupied in it
    behind = torch.tensor([[float(robot.position[0]) - 1.5, 0.0625, 0.5]], device=robot.map.device)   # in the wall y = 0
    assert int(robot.map.log_odds(behind)[1]) == 2, "the wall a metre and a half behind the robot is still in the map"
    return robot, records


def team(steps=10, margin=(14, 2, 2), device="cuda:0", verbose=True):
    """Two robots from opposite ends, their maps fused -> (the fused map, its clusters)."""
    world = make_world(torch.device(device))
    a = Robot(world, START, +1, margin)
    b = Robot(world, (LENGTH - START[0], START[1], START[2]), -1, margin)
    for _ in range(steps):
        a.step()
        b.step()
    fused = merge_maps([a.map, b.map])                      # mode 'confident': the stronger belief wins
    other = merge_maps([b.map, a.map])
    assert torch.equal(fused.buf, other.buf) and torch.equal(fused.occupied.buf, other.occupied.buf), "any merge order gives the same map"
    known = int((fused.dense() != ops.EVID_UNKNOWN).sum())
    assert known >= max(a.known(), b.known()) and fused.dims[0] > BOX[0]
    clusters = frontier_clusters(fused, min_size=4)
    if verbose:
        print(f"team: boxes from x = {float(a.map.origin[0]):.3f} and x = {float(b.map.origin[0]):.3f} fused into one of {fused.dims} voxels "
              f"from x = {float(fused.origin[0]):.3f}: {known} known voxels ({a.known()} and {b.known()} apart), {clusters.n} frontier clusters")
        for i in range(min(clusters.n, 6)):
            c = clusters.centroids[i].tolist()
            print(f"         cluster {int(clusters.ids[i]):3d}: {int(clusters.sizes[i]):4d} voxels around ({c[0]:.2f}, {c[1]:.2f}, {c[2]:.2f})")
    lo, hi = float(a.position[0]), float(b.position[0])
    if clusters.n:
        big = float(clusters.centroids[0, 0])
        assert lo - 3.0 < big < hi + 3.0, "the largest opening of the fused map lies between the two robots"
    return fused, clusters


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=34)
    ap.add_argument("--margin", type=int, default=14, help="voxels the robot keeps from the box's ends along the corridor")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device: the map and the planning chain have no CPU fallback")
    margin = (args.margin, 2, 2)
    robot, records = roll(args.steps, margin)
    print(f"the map moved {robot.moves} times and stayed {robot.map.dims} voxels")
    team(margin=margin)
    return records


if __name__ == "__main__":
    main()
