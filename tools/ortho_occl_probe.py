#!/usr/bin/env python3
"""Probe: what the occlusion-tested mosaic (OrthoSettings(occlusion_test=True),
k_ortho_occl_backward) costs beside the plain mosaic on the same inputs, in the same run.

Workloads: cfg3's mosaic inputs (bench.py: 10000 x 10000 cells at 0.25 m, the DSM of its 50 M-point
cloud, 249 frames of 1920 x 1080 from 700 m) and the same with synthetic blocks on the surface (20 m
high, 10 m x 10 m, one per 100 m x 100 m: the surface then comes from outside and the march's
height cut-off from the kernel's own reduction).  Per workload the two mosaics alternate, ROUNDS
rounds after one warm-up round each; times are the `k_ortho_backward` slot of
amhip_ctx_kernel_time (HIP events around the call's kernels).  One JSON line on stdout.

  python tools/ortho_occl_probe.py [--side 10000] [--rounds 7] [--margin 0.1]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import aerial_mapper_amd as A
from aerial_mapper_amd import hip_lib, synth

ap = argparse.ArgumentParser()
ap.add_argument("--side", type=int, default=10000)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--margin", type=float, default=0.1)
args = ap.parse_args()

dev = torch.device("cuda", 0)
side, res, W, H, F, f, alt = args.side, 0.25, 1920, 1080, 249, 1400.0, 700.0
L = side * res
n_pts = int(50_000_000 * (side / 10000.0) ** 2)
pts = synth.make_points_torch(n_pts, (L / 2.0 + 2.0, L / 2.0 + 2.0), 43, dev)
frames = synth.make_frames_torch(F, H, W, 1, 44, dev)
poses = synth.make_lawnmower_poses(F, L / 2.0, alt, 44, tilt_deg=5.0)
ncam = A.NCamera(f, f, (W - 1) / 2.0, (H - 1) / 2.0, W, H)
SLOT = "k_ortho_backward"


def stats(ts):
    ts = sorted(ts)
    return {"median_ms": round(ts[len(ts) // 2], 4), "min_ms": round(ts[0], 4), "max_ms": round(ts[-1], 4)}


out = {"probe": "ortho_occl_probe", "build_id": hip_lib.build_id(), "side": side, "resolution": res, "frames": F,
       "margin_m": args.margin, "rounds": args.rounds, "timing": "amhip_ctx_kernel_time, slot " + SLOT,
       "workloads": {}}
with A.AerialGridMap(A.GridMapSettings(0.0, 0.0, L, L, res)) as m:
    dsm = A.Dsm(A.DsmSettings(interpolation_radius=1), m)
    plain = A.OrthoBackwardGrid(ncam, A.OrthoSettings(), m)
    occl = A.OrthoBackwardGrid(ncam, A.OrthoSettings(occlusion_test=True, occlusion_margin_m=args.margin), m)
    occl_inf = A.OrthoBackwardGrid(ncam, A.OrthoSettings(occlusion_test=True, occlusion_margin_m=float("inf")), m)
    m.enable_timing(True)
    dsm.process(pts, m)
    surface = m.get("elevation")
    blocks = surface.copy()
    cells = int(round(10.0 / res))            # a block's edge
    pitch = int(round(100.0 / res))
    for j0 in range(pitch // 2, side - cells, pitch):
        for i0 in range(pitch // 2, side - cells, pitch):
            blocks[j0:j0 + cells, i0:i0 + cells] += np.float32(20.0)

    def prepare(name):
        m.reset()
        if name == "cfg3":
            dsm.process(pts, m)               # (the context knows the range of its heights)
        else:
            m.set("elevation", blocks)        # (heights from outside: the kernel reduces the maximum)
        m.synchronize()

    for name in ("cfg3", "cfg3_blocks"):
        # plain_exact_unpruned: the plain mosaic as the new kernel has to fold (every pair in the
        # reference's arithmetic, the frame list not pruned); occl_inf: margin +inf -- every
        # accepted pair marches to the cut-off and none is occluded
        ARMS = (("plain", plain), ("plain_exact_unpruned", plain), ("occl_inf", occl_inf), ("occl", occl))
        ts = {which: [] for which, _ in ARMS}
        layers = {}
        for rnd in range(args.rounds + 1):    # (round 0: warm-up)
            for which, mosaic in ARMS:
                prepare(name)
                exact = which == "plain_exact_unpruned"
                hip_lib.set_tuning("ortho_exact_fold", "1" if exact else None)
                hip_lib.set_tuning("ortho_no_prune", "1" if exact else None)
                m.timing_reset()
                mosaic.process(poses, frames, m)
                ms, launches = m.kernel_times()[SLOT]
                if rnd:
                    ts[which].append(ms)
                elif which in ("plain", "occl"):
                    layers[which] = m.get("observation_index")
        a, b = layers["plain"], layers["occl"]
        differ = ~((a == b) | (np.isnan(a) & np.isnan(b)))
        out["workloads"][name] = {
            "plain": stats(ts["plain"]), "occl": stats(ts["occl"]),
            "plain_exact_unpruned": stats(ts["plain_exact_unpruned"]), "occl_margin_inf": stats(ts["occl_inf"]),
            "ratio_of_medians": round(stats(ts["occl"])["median_ms"] / stats(ts["plain"])["median_ms"], 3),
            "cells_observation_index_differs": int(differ.sum()),
            "cells_left_initial_by_occlusion": int((np.isnan(b) & ~np.isnan(a)).sum()),
            "coverage_plain": round(float((~np.isnan(a)).mean()), 4)}
print(json.dumps(out))
