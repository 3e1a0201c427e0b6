#!/usr/bin/env python3
"""Localising in a known map with a particle filter: tracking from a rough prior, and a global start.

The scene is that of examples/scan_matching_sample.py: a robot circles the doorway room and scans all round at every step.  First the
map is made — an evidence map of the scans placed at their true poses.  Then the robot goes round again and has to say where it is:

  tracking      tools.particle_filter is seeded around a prior that is 12 cm and 4 degrees off; at every step it is told the
                odometry's increment in the body frame — which drifts, as in the scan-matching sample — with its noise, weighs its
                particles by the scan and resamples where the weights have collapsed.  Printed per step: how far dead reckoning from
                the same prior and the filter's weighted mean are from the truth.
  global start  a second filter knows nothing: pf.seed_positions(map.free.export()) spreads it over every voxel the map knows to be
                free, with headings all round, and the same steps follow.  Whether it finds the robot depends on how many particles
                fall near the truth: the sample reports the outcome and asserts nothing about it.

    python examples/particle_localisation_sample.py [--steps 8] [--particles 4096]
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from closed_loop_exploration_sample import GEOMETRY, world_points  # noqa: E402
from scan_matching_sample import DRIFT, place, sense, true_path  # noqa: E402
from trajectory_optimization_amd.tools import evidence_map, occupancy_grid, particle_filter  # noqa: E402

PRIOR_OFF, PRIOR_YAW_OFF = (0.09, -0.08, 0.0), np.deg2rad(4.0)     # the tracking prior's error
PRIOR_SIGMA = ((0.15, 0.15, 0.05), np.deg2rad(5.0))
MOTION_SIGMA = (0.06, 0.06, 0.02, np.deg2rad(2.0))                 # covers the odometry's drift per step
EVERY = 8                                                          # returns of a scan the filter looks at: one in eight
GLOBAL_PARTICLES = 1 << 17


def body_delta(p0, yaw0, p1, yaw1):
    """The motion from pose 0 to pose 1 as the robot at pose 0 sees it -> (dx, dy, dz, dyaw)."""
    c, s = np.cos(yaw0), np.sin(yaw0)
    d = np.asarray(p1) - np.asarray(p0)
    return (c * d[0] + s * d[1], -s * d[0] + c * d[1], d[2], yaw1 - yaw0)


def yaw_error(a, b):
    return abs((a - b + np.pi) % (2.0 * np.pi) - np.pi)


def run(steps=8, n=4096, device="cuda:0", verbose=True, seed=1):
    """-> dict(tracking: per step (dead reckoning's error, the filter's error) in metres; tracking_yaw: the same in radians; global:
    per step the global filter's error in metres; resolution)."""
    device = torch.device(device)
    world = occupancy_grid(device=device, **GEOMETRY)
    world.insert(torch.from_numpy(world_points()).to(device))
    truth, yaws = true_path(steps + 1)
    scans = [sense(world, truth[i], yaws[i], device) for i in range(steps + 1)]
    m = evidence_map(occupancy_grid(device=device, **GEOMETRY))
    for i in range(steps + 1):                                    # the map, made with the true poses
        m.integrate(torch.as_tensor(truth[i], dtype=torch.float32, device=device)[None, :], place(scans[i], truth[i], yaws[i]))
    # the odometry: the truth plus a drift that accumulates; the filter is told its increments
    odom_p = [truth[i] + i * np.asarray(DRIFT["step"]) for i in range(steps + 1)]
    odom_yaw = [yaws[i] + i * DRIFT["yaw"] for i in range(steps + 1)]
    deltas = [body_delta(odom_p[i - 1], odom_yaw[i - 1], odom_p[i], odom_yaw[i]) for i in range(1, steps + 1)]

    pf = particle_filter(m, n, seed=seed)
    prior_p, prior_yaw = truth[0] + np.asarray(PRIOR_OFF), yaws[0] + PRIOR_YAW_OFF
    pf.seed_gaussian(prior_p, prior_yaw, *PRIOR_SIGMA)
    free = m.free.export()[1]
    gf = particle_filter(m, GLOBAL_PARTICLES, seed=seed + 1).seed_positions(free)
    dead_p, dead_yaw = prior_p.copy(), float(prior_yaw)
    tracking, tracking_yaw, glob = [], [], []
    for i in range(1, steps + 1):
        pts = scans[i][::EVERY].contiguous()
        d = deltas[i - 1]
        c, s = np.cos(dead_yaw), np.sin(dead_yaw)
        dead_p = dead_p + np.array([c * d[0] - s * d[1], s * d[0] + c * d[1], d[2]])
        dead_yaw += d[3]
        est = pf.predict(d, MOTION_SIGMA).weigh(pts).estimate()
        pf.resample(0.5)
        g = gf.predict(d, MOTION_SIGMA).weigh(pts).estimate()
        gf.resample(0.5)
        tracking.append((float(np.linalg.norm(dead_p - truth[i])), float(np.linalg.norm(est.pose - truth[i]))))
        tracking_yaw.append((yaw_error(dead_yaw, yaws[i]), yaw_error(est.yaw, yaws[i])))
        glob.append(float(np.linalg.norm(g.pose - truth[i])))
        if verbose:
            print(f"step {i}: {pts.shape[0]} returns  dead reckoning off by {tracking[-1][0]:.3f} m {np.rad2deg(tracking_yaw[-1][0]):.1f} deg  "
                  f"filter off by {tracking[-1][1]:.3f} m {np.rad2deg(tracking_yaw[-1][1]):.1f} deg (n_eff {est.n_eff:.0f}, best sees "
                  f"{est.known}/{est.used})  global start off by {glob[-1]:.3f} m (n_eff {g.n_eff:.0f})")
    return dict(tracking=tracking, tracking_yaw=tracking_yaw, resolution=float(m.resolution), free_voxels=int(free.shape[0]), **{"global": glob})


def check(result):
    """The sample's own assertions, on tracking only: at the last step the filter is within a voxel and a half and three degrees of
    the truth, and nearer than dead reckoning from the same prior."""
    dead, est = result["tracking"][-1]
    dead_yaw, est_yaw = result["tracking_yaw"][-1]
    assert est <= 1.5 * result["resolution"] and est_yaw <= np.deg2rad(3.0), result
    assert est < dead, result


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--particles", type=int, default=4096)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("needs a HIP device: the map and the filter have no CPU fallback")
    result = run(args.steps, args.particles)
    check(result)
    print(f"tracking: the filter ends {result['tracking'][-1][1]:.3f} m from the truth, dead reckoning {result['tracking'][-1][0]:.3f} m")
    print(f"global start over {result['free_voxels']} free voxels with {GLOBAL_PARTICLES} particles: ends {result['global'][-1]:.3f} m from the truth"
          f" ({'found the robot' if result['global'][-1] <= 1.5 * result['resolution'] else 'did not find the robot'})")
    return result


if __name__ == "__main__":
    main()
