#!/usr/bin/env python3
"""Probe: what the blended mosaic (OrthoSettings(blend=True), k_ortho_blend_backward) costs beside
the unblended mosaics on the same inputs, in the same run.

Workload: cfg3's mosaic inputs (bench.py: 10000 x 10000 cells at 0.25 m, the DSM of its 50 M-point
cloud, 249 gray frames of 1920 x 1080 from 700 m).  The modes alternate in one process, ROUNDS
rounds after one warm-up round; every call starts from a reset map (so every blended call restarts
and writes its sums); times are the `k_ortho_backward` slot of amhip_ctx_kernel_time (HIP events
around the call's kernels).  One JSON line on stdout.

  python tools/ortho_blend_probe.py [--side 10000] [--rounds 7] [--margin 0.1] [--sharpness 2]
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
ap.add_argument("--sharpness", type=int, default=2)
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


out = {"probe": "ortho_blend_probe", "build_id": hip_lib.build_id(), "side": side, "resolution": res, "frames": F,
       "margin_m": args.margin, "sharpness": args.sharpness, "rounds": args.rounds,
       "timing": "amhip_ctx_kernel_time, slot " + SLOT}
with A.AerialGridMap(A.GridMapSettings(0.0, 0.0, L, L, res)) as m:
    dsm = A.Dsm(A.DsmSettings(interpolation_radius=1), m)

    def mosaic(**kw):
        return A.OrthoBackwardGrid(ncam, A.OrthoSettings(**kw), m)

    occl = dict(occlusion_test=True, occlusion_margin_m=args.margin)
    blend = dict(blend=True, blend_sharpness=args.sharpness)
    # plain_exact_unpruned: the plain mosaic as the blended kernel has to fold (every pair in the
    # reference's arithmetic, the frame list not pruned) -- the like-for-like fold
    ARMS = (("plain", mosaic()), ("plain_exact_unpruned", mosaic()), ("occl", mosaic(**occl)),
            ("blend", mosaic(**blend)), ("blend_occl", mosaic(**blend, **occl)))
    m.enable_timing(True)
    ts = {which: [] for which, _ in ARMS}
    layers = {}
    for rnd in range(args.rounds + 1):        # (round 0: warm-up)
        for which, arm in ARMS:
            m.reset()
            dsm.process(pts, m)               # (the context knows the range of its heights)
            m.synchronize()
            exact = which == "plain_exact_unpruned"
            hip_lib.set_tuning("ortho_exact_fold", "1" if exact else None)
            hip_lib.set_tuning("ortho_no_prune", "1" if exact else None)
            m.timing_reset()
            arm.process(poses, frames, m)
            ms, launches = m.kernel_times()[SLOT]
            if rnd:
                ts[which].append(ms)
            elif which in ("plain", "blend"):
                layers[which] = (m.get("observation_index"), m.get("ortho"))
    for which, _ in ARMS:
        out[which] = stats(ts[which])
    (ia, oa), (ib, ob) = layers["plain"], layers["blend"]
    seen = ~np.isnan(ia)
    out["blend_over_plain"] = round(out["blend"]["median_ms"] / out["plain"]["median_ms"], 3)
    out["blend_over_plain_exact_unpruned"] = round(
        out["blend"]["median_ms"] / out["plain_exact_unpruned"]["median_ms"], 3)
    out["blend_occl_over_occl"] = round(out["blend_occl"]["median_ms"] / out["occl"]["median_ms"], 3)
    out["coverage_plain"] = round(float(seen.mean()), 4)
    out["cells_observation_index_differs"] = int((~((ia == ib) | (np.isnan(ia) & np.isnan(ib)))).sum())
    out["cells_ortho_differs"] = int((oa != ob).sum())
    # derived, not measured: the sums a call reads and writes, gray (2 doubles a cell); a restarted
    # cell is only written, a continued one read and written
    out["accumulator_bytes_per_cell_and_call"] = {"gray_restart": 16, "gray": 32, "colour_restart": 32, "colour": 64}
    out["accumulator_bytes_this_call"] = int(16 * m.rows * m.cols)
print(json.dumps(out))
