#!/usr/bin/env python3
"""bench.py -- DSM + backward-grid orthomosaic throughput on MI355X.

  python bench.py --gpus N --steps K --warmup W
  (N > 1: under python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N ..., or
   plainly -- bench.py then starts the N ranks itself; it never prints a line for fewer GPUs
   than --gpus asked for)

One "step" = one pass of the hot path over one batch of synthetic input that is
already resident in HBM:  AerialGridMap::initialize() (layer reset) ->
dsm::Dsm::process (point cloud -> elevation) -> ortho::OrthoBackwardGrid::process
(249 frames -> most-nadir view per cell).  Metric = BASELINE.json's
"Mcells/s (DSM+ortho)": grid cells finished per second, whole job.

Workload at N = 1 (default `cfg3`, BASELINE.json configs[2] = configs[1]'s DSM
+ the ortho layer): 50 M points -> 10 000 x 10 000 cells @ 0.25 m, 249 frames
1920x1080 8UC1.  With N ranks every rank owns one such tile of a larger survey
(weak scaling, no data-path collective: cells are independent once a rank
holds the points within the last fallback radius of its tile, which the
synthetic generator hands it directly).

Prints ONE JSON line on rank 0: metric, value, unit, higher_is_better, dtype, ms_per_step (one
timed step), the per-kernel HIP-event times of the timed steps and `roofline` (dominant kernel,
algorithmic bytes / measured HIP-event time, vs 8 TB/s HBM).  That is all a plain run does: set
up, warm up, time --steps steps, print.  --dump-outputs DIR also writes the layers of the last
timed step (see its help).

--full adds everything else, after the timed steps: `cpu_baseline` (the CPU oracle timed on a
bounded sample of the same workload on the host's cores) with its `parity_sample`, the other
arithmetic mode, `launch_skips`, `rough_terrain`, the host-buffer route (`pcie_inclusive`,
N > 1: `session_route`), `other_workloads` and, N > 1, the `preflight`.

`value` is the library's DEFAULT arithmetic: the FP64 gather (the reference's doubles,
dsm.cc:160-172).  With --full the opt-in single-precision mode is timed in the same run and
reported as the extra object `fast_mode`, with its own parity sample and roofline.

`value` is the call the reference's hosts make (main-dsm.cc:103-107, main-ortho-backward-grid.cc:
128-141: ONE process() per process): every timed DSM call counts, sorts and gathers its cloud from
scratch -- no data pass is skipped because the cloud repeats (the round-4 plan reuse is gone from
the library).  The N > 1 ranks run the same pipeline.  The one thing a repeated call still takes
from its predecessor is a LAUNCH policy: kernels whose work lists were empty last time (the
capacity-class gathers, the big-sub-partition placement) are not launched; the extra object
`launch_skips` (--full) times the same steps with every such kernel launched (tuning key
no_launch_skips: what a context's very first call runs) so the difference is on the line.

The parity sample of --full is the WHOLE map by default (--cpu-sample-side 10000: the CPU oracle --
the reference's loops restated over its own vendored nanoflann -- on all 1e8 cells, ~1 min of host time).
--workload cfg1 = BASELINE.json configs[0] exactly (1 M points, std::mt19937_64 seed 42,
1000 x 1000 cells @ 1.0 m, interpolation_radius 1: 4 % of the cells take the fallback ladder).
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: 8.0 TB/s spec

# --dump-outputs: cells kept per layer (5 layers + their finite masks: 10 x 2^20 x 4 B = 40 MiB at
# most) and the sample's seed
DUMP_CELLS = 1 << 20
DUMP_SEED = 20240607

WORKLOADS = {
    # name: (cells per side, resolution, points, frames, W, H)
    # BASELINE.json configs[0] / SURVEY.md 8d cfg1, exactly: std::mt19937_64(42), x, y ~ U(-500, 500)
    "cfg1": dict(side=1000, res=1.0, points=1_000_000, frames=0, W=1920, H=1080,
                 f=1400.0, altitude=700.0, mt19937_seed=42,
                 desc="1M pts (std::mt19937_64 seed 42, U(-500,500)^2) -> 1000x1000 @1.0m DSM "
                      "(radius_sq=1: ~3.1 neighbours per cell, ~4 % of the cells on the fallback ladder)"),
    "cfg3": dict(side=10000, res=0.25, points=50_000_000, frames=249, W=1920, H=1080,
                 f=1400.0, altitude=700.0,
                 desc="50M pts -> 10000x10000 @0.25m DSM (radius_sq=1) + OrthoBackwardGrid, "
                      "249 frames 1920x1080 8UC1"),
    "cfg2": dict(side=10000, res=0.25, points=50_000_000, frames=0, W=1920, H=1080,
                 f=1400.0, altitude=700.0,
                 desc="50M pts -> 10000x10000 @0.25m DSM only (radius_sq=1)"),
    "small": dict(side=2000, res=0.25, points=2_000_000, frames=24, W=1920, H=1080,
                  f=1400.0, altitude=700.0,
                  desc="2M pts -> 2000x2000 @0.25m DSM + ortho, 24 frames (smoke-size)"),
    # BASELINE.json configs[3] / configs[4]: ONE fixed survey cut over the ranks (strong scaling;
    # 2 x 4 windows of 20000 x 10000 cells on 8 GPUs; the whole map on one GPU at N = 1)
    "cfg4": dict(side=40000, res=0.25, points=400_000_000, frames=0, W=1920, H=1080,
                 f=1400.0, altitude=700.0, fixed_map=True,
                 desc="400M pts -> 40000x40000 @0.25m DSM (radius_sq=1), tiled over the GPUs, halo "
                      "points exchanged with the neighbouring windows over RCCL"),
    "cfg5": dict(side=40000, res=0.25, points=400_000_000, frames=2000, batch=64, W=1920, H=1080,
                 f=1400.0, altitude=700.0, fixed_map=True,
                 desc="incremental mosaic: 2000 frames of a 10 km lawn-mower flight appended in "
                      "64-frame batches onto the resident layers of the 40000x40000 @0.25m map "
                      "(DSM of the 400M-point cloud built once, untimed); a step = one batch"),
    "small5": dict(side=4096, res=0.25, points=4_000_000, frames=160, batch=64, W=1920, H=1080,
                   f=1400.0, altitude=700.0, fixed_map=True,
                   desc="incremental mosaic like cfg5 at test size: 160 frames appended in 64-frame batches "
                        "(64 + 64 + 32) onto the resident layers of a 4096x4096 @0.25m map"),
    "small4": dict(side=4096, res=0.25, points=4_000_000, frames=0, W=1920, H=1080,
                   f=1400.0, altitude=700.0, fixed_map=True,
                   desc="4M pts -> 4096x4096 @0.25m DSM, tiled like cfg4 (test size)"),
}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workload", default="cfg3", choices=sorted(WORKLOADS))
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-sample-side", type=int, default=10000,
                    help="cells per side of the corner sub-tile the CPU oracle is timed on and "
                         "the GPU layers are compared with (default: the whole 10000 x 10000 map of cfg3, "
                         "~1 min of host time; 4000 for a quick run)")
    ap.add_argument("--colored", action="store_true", help="8UC3 frames / colored_ortho")
    ap.add_argument("--host-path", action="store_true", default=True,
                    help="(default with --full at N = 1) also time ONE pass through the host-buffer (drop-in) "
                         "entry points, PCIe transfers included (reported as pcie_inclusive, never "
                         "as value)")
    ap.add_argument("--no-host-path", dest="host_path", action="store_false")
    ap.add_argument("--knn", type=int, default=0,
                    help="OPTIONAL capped DSM mode (only the k nearest points of a cell's search; "
                         "not a reference code path): a separately reported extra, never the graded line")
    ap.add_argument("--verify", action="store_true",
                    help="N > 1, small workloads: after the timed steps gather the cloud and every "
                         "window's elevation on rank 0 and compare with ONE full-map DSM there")
    ap.add_argument("--dsm-mode", default="exact", choices=["fast", "exact"],
                    help="arithmetic of the DSM gather in the timed steps behind `value`: exact = "
                         "FP64 (the library's default: the reference's arithmetic, dsm.cc:160-172, and "
                         "its floats), fast = single precision under exact guards (opt-in mode of the "
                         "library, within the north_star's 1e-4 m).  The other mode is timed in the "
                         "same run and reported beside it (`fast_mode` / `exact_mode`)")
    ap.add_argument("--no-second-mode", action="store_true", help="skip the other mode's loop")
    ap.add_argument("--no-rough-terrain", action="store_true",
                    help="skip the rough-terrain extra (N = 1: 25 m steps in 20 %% of the gather tiles)")
    ap.add_argument("--window-parity", action="store_true",
                    help="N = 1, one fixed survey (cfg4 / small4): after the timed steps compare four "
                         "600 x 600-cell windows of the elevation layer (three corners and the middle) "
                         "with the CPU oracle's DSM of those windows")
    ap.add_argument("--no-other-workloads", action="store_true",
                    help="--full run (cfg3, N = 1): skip the child runs of the other BASELINE configs "
                         "(`other_workloads`)")
    ap.add_argument("--no-preflight", action="store_true",
                    help="N > 1, --full: skip the small verified step in front of the timed ones")
    ap.add_argument("--route", default="auto", choices=["auto", "ranks", "session"],
                    help="`value` is always the one-process-per-GPU route.  session: rank 0 ALSO times "
                         "(after the timed steps) one pass of the whole map through ONE host process "
                         "driving all N devices -- amhip_session on host buffers, the route "
                         "AERIAL_MAPPER_HIP_DEVICES gives an unchanged C++ host (main-dsm.cc:103-107, "
                         "main-ortho-backward-grid.cc:128-141) -- reported as `session_route` (N = 1: "
                         "`pcie_inclusive`, the same thing), never as value.  auto (default): the same "
                         "with --full, when the host has the memory for the whole map's matrices; ranks: never")
    ap.add_argument("--session-child", type=int, default=0, help=argparse.SUPPRESS)   # (internal: see session_route_all)
    ap.add_argument("--map-origin", default="0,0",
                    help="easting,northing of the map centre (default 0,0; e.g. 464980.25,5272690.5 "
                         "puts the same workload at UTM magnitudes)")
    ap.add_argument("--full", action="store_true",
                    help="also run everything beside the headline figure: the CPU baseline and its parity "
                         "sample, the other arithmetic mode, launch_skips, rough_terrain, the host-buffer "
                         "route (pcie_inclusive / session_route), other_workloads and, for N > 1, the "
                         "preflight.  Without it a run sets up, warms up, times the steps and prints its line "
                         "(the --no-* options above switch single parts of --full off)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write the layers the last timed step produced (elevation; "
                         "with frames also elevation_angle, num_observations, observation_index and ortho / "
                         "colored_ortho) as DIR/<layer>.npy, float32, shaped (cols, rows) like "
                         "AerialGridMap.get, every value finite: a cell without a finite value (NaN: a layer's reset value "
                         "where nothing was written: elevation without points, observation_index without a "
                         "view) is written as 0.0, and DIR/<layer>_finite.npy (same shape) holds 1.0 where "
                         "the layer holds a finite value, 0.0 elsewhere.  A layer of more than %d cells is "
                         "written as a fixed 1-D sample of %d of its cells (flat indices into that array "
                         "drawn by numpy PCG64 seed %d, sorted), so that all files stay within 40 MiB.  "
                         "N > 1: DIR/rank<r>_<layer>.npy per rank window" % (DUMP_CELLS, DUMP_CELLS, DUMP_SEED))
    a = ap.parse_args()
    if a.knn:   # (the CPU baseline / parity sample are the REFERENCE's algorithm: not this mode)
        a.no_cpu_baseline = True
        a.host_path = False
    return a


def cpu_baseline(args, wl, map_, pts_dev, frames_dev, poses, ncam, tile_center):
    """Time the CPU oracle on a corner sub-tile of this rank's workload and keep its layers for the
    parity check.  The oracle = the reference's loops restated (oracle/amo_dsm.cc, amo_ortho.cc) over
    the reference's OWN vendored nanoflann (oracle/_ref/liboracle_ref.so: nanoflann.hpp compiles by
    itself from where it lies) -- `kind: port`.  dsm.cc / ortho-backward-grid.cc themselves need
    Eigen, grid_map, glog, aslam, minkindr and OpenCV, which the image lacks: unbuildable here by
    the task's rules (a build over stand-in headers is not a reference build; the one under
    oracle/refkit is kept as a consistency check of the restatement -- tests/test_reference_loops.py
    -- and is neither timed nor compared with here).
    Threads: std::thread::hardware_concurrency() like utils::parFor (dsm.cc:178), and -- on a smaller
    corner, SURVEY 8(d) -- one thread per CPU of the cgroup quota beside it."""
    import numpy as np
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_ffi as O
    which = "ref" if O.have_ref() else "port"
    side, res = wl["side"], wl["res"]
    L = side * res
    F = wl["frames"]
    cores, quota = usable_cpus()
    threads = os.cpu_count() or 1
    cam = None
    frames_host = None
    if F:
        frames_host = [f for f in frames_dev.cpu().numpy()]
        cam = O.Camera()
        cam.fu, cam.fv, cam.cu, cam.cv = ncam.camera.fu, ncam.camera.fv, ncam.camera.cu, ncam.camera.cv
        cam.width, cam.height = ncam.camera.width, ncam.camera.height

    def run(s, num_threads):
        # sub-tile = cells [0,s) x [0,s) of the big grid: its cell centres are
        # x_i = base_x - res*i with base_x = cx + L/2 - res/2 (all dyadic here)
        sub_len = s * res
        sub_cx = tile_center[0] + L / 2.0 - sub_len / 2.0
        sub_cy = tile_center[1] + L / 2.0 - sub_len / 2.0
        g = O.make_grid(sub_len, sub_len, res, sub_cx, sub_cy, which=which)
        assert g.rows == s and g.cols == s
        halo = 3.0
        x, y = pts_dev[:, 0], pts_dev[:, 1]
        keep = (x > sub_cx - sub_len / 2 - halo) & (x < sub_cx + sub_len / 2 + halo) & \
               (y > sub_cy - sub_len / 2 - halo) & (y < sub_cy + sub_len / 2 + halo)
        sub_pts = pts_dev[keep].cpu().numpy()
        rc, elev, (t_build, t_cells) = O.dsm_process(sub_pts, g, 1, 0.0, 0.0, which=which,
                                                     num_threads=num_threads)
        assert rc == 0
        t_ortho = 0.0
        layers = O.new_layers(g)
        layers["elevation"] = elev
        if F:
            t0 = time.time()
            rc = O.ortho_process(g, cam, poses, ncam.T_C_B, frames_host, layers, colored=args.colored,
                                 which=which, num_threads=num_threads)
            assert rc == 0
            t_ortho = time.time() - t0
        return g, sub_pts.shape[0], elev, layers, t_build, t_cells, t_ortho

    s = min(args.cpu_sample_side, side)
    g, npts, elev, layers, t_build, t_cells, t_ortho = run(s, 0)
    total = t_build + t_cells + t_ortho
    out = {"value": round(s * s / total / 1e6, 4), "unit": "Mcells/s", "cores": cores,
           "threads": threads, "cpu_quota": quota, "kind": "port",
           "reference_code": {"ref": "kd-tree: the reference's vendored nanoflann.hpp (v1.2.2) compiled unchanged "
                                     "from /root/reference; loops: restated (oracle/amo_dsm.cc, amo_ortho.cc)",
                              "port": "none (restated loops, restated kd-tree)"}[which],
           "sample": ("%dx%d-cell corner sub-tile of the workload (%d pts incl. 3 m halo, all %d frames brute "
                      "force like the reference): kd-tree build %.2fs (1 thread, dsm.cc:36-52) + cell loop "
                      "%.2fs + mosaic %.2fs, std::thread x hardware_concurrency (= %d) like utils::parFor; "
                      "the reference's constructors' per-cell tables (dsm.cc:20-34, ortho-backward-grid.cc:23-40) "
                      "are not part of the restatement: ctor_s = 0"
                      % (s, s, npts, F, t_build, t_cells, t_ortho, threads)),
           "dsm_s": round(t_build + t_cells, 3), "ortho_s": round(t_ortho, 3),
           "ctor_s": 0.0, "kdtree_build_s": round(t_build, 3), "query_s": round(t_cells, 3)}
    refs = {"s": s, "elev": elev, "layers": layers, "grid": g, "cam": cam, "frames_host": frames_host,
            "which": which}
    # the same with one thread per CPU of the quota, on a corner of at most 4000 x 4000 cells
    if cores < threads:
        s2 = min(4000, s)
        _, npts2, _, _, b2, c2, o2 = run(s2, cores)
        out["threads_quota_run"] = {"threads": cores, "cells": s2 * s2, "points": npts2,
                                    "kdtree_build_s": round(b2, 3), "query_s": round(c2, 3),
                                    "ortho_s": round(o2, 3),
                                    "Mcells_per_s": round(s2 * s2 / (b2 + c2 + o2) / 1e6, 4)}
    return refs, out


def usable_cpus():
    """(CPUs this process may keep busy, the cgroup CPU quota in CPUs or None)."""
    import math
    n = os.cpu_count() or 1
    try:
        n = min(n, len(os.sched_getaffinity(0)))
    except (AttributeError, OSError):
        pass
    quota = None
    try:
        a, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if a != "max":
            quota = float(a) / float(period)
    except (OSError, ValueError):
        try:
            q = float(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            per = float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0 and per > 0:
                quota = q / per
        except (OSError, ValueError):
            pass
    if quota:
        n = min(n, max(1, int(math.ceil(quota))))
    return n, quota


def parity_against(refs, args, map_, poses, ncam, F):
    """GPU layers of the sub-tile against the oracle's (already computed) result."""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_ffi as O
    s, elev, layers = refs["s"], refs["elev"], refs["layers"]
    gpu_elev = map_.get("elevation")[:s, :s]
    ok = ~np.isnan(elev)
    same = (gpu_elev.view(np.uint32) == elev.view(np.uint32)) | (np.isnan(gpu_elev) & ~ok)
    parity = {"cells": int(s * s),
              "dsm_nan_pattern_equal": bool(np.array_equal(np.isnan(gpu_elev), ~ok)),
              "dsm_max_abs_err_m": float(np.abs(gpu_elev[ok].astype(np.float64) - elev[ok]).max())
              if ok.any() else 0.0,
              "dsm_bit_identical_frac": round(float(same.mean()), 9)}
    if F:
        names = ("observation_index", "colored_ortho" if args.colored else "ortho")
        for name in names:
            a = map_.get(name)[:s, :s]
            b = layers[name]
            eq = (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
            parity[name + "_mismatch_cells"] = int((~eq).sum())
        if any(parity[k] for k in parity if k.endswith("_mismatch_cells")):
            # The reference's mosaic stands on the REFERENCE's heights, the GPU's on its own
            # (single-precision gather: within 1e-4 m, not bit-identical).  A height that
            # moved by one float spacing can carry a keypoint across a pixel boundary; whether the
            # mosaic kernel itself is exact is decided on equal inputs: the reference's loop once
            # more, on the GPU's heights.
            layers2 = O.new_layers(refs["grid"])
            layers2["elevation"] = np.ascontiguousarray(gpu_elev)
            rc = O.ortho_process(refs["grid"], refs["cam"], poses, ncam.T_C_B, refs["frames_host"],
                                 layers2, colored=args.colored, which=refs["which"])
            assert rc == 0
            for name in names:
                a = map_.get(name)[:s, :s]
                b = layers2[name]
                eq = (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
                parity[name + "_mismatch_cells_on_equal_heights"] = int((~eq).sum())
            parity["note"] = ("*_mismatch_cells: GPU DSM + mosaic against the oracle's DSM + mosaic (the "
                              "heights differ by <= dsm_max_abs_err_m); *_on_equal_heights: the "
                              "oracle's mosaic loop fed the GPU's heights")
    return parity


def rough_terrain(args, A, m, pts, dsm, side, res, tile_center, L):
    """What a rough scene costs: the same cloud with a 25 m step through the
    middle of 20 % of the 64 x 16-cell gather tiles (walls / canopy edges).  The single-precision
    gather's per-tile error bound has no room there (height range beyond ~15 m at 400 m), so
    those tiles -- and the neighbours whose halo ring reaches into them -- go to the FP64 kernel.
    DSM calls only (the mosaic does not depend on the mode)."""
    import torch
    dev = pts.device
    rough = pts.clone()
    bx = tile_center[0] + L / 2.0        # x of the map's upper edge (cell 0 starts here)
    by = tile_center[1] + L / 2.0
    u = (bx - rough[:, 0]) / (64 * res)
    v = (by - rough[:, 1]) / (16 * res)
    ti, tj = torch.floor(u).to(torch.int64), torch.floor(v).to(torch.int64)
    h = (ti * 73856093) ^ (tj * 19349663)
    chosen = (h % 5) == 0
    step_up = chosen & ((u - torch.floor(u)) > 0.5)
    rough[:, 2] += 25.0 * step_up.to(torch.float64)
    frac_tiles = float(chosen.double().mean().item())
    del u, v, ti, tj, h, chosen, step_up
    res_out = {"scene": "cfg's cloud + a 25 m step through the middle of one in five of the 64x16-cell "
                        "gather tiles (%.3f of the points lie in such a tile)" % frac_tiles}
    for mode in ("fast", "exact"):
        m.set_dsm_precision(mode == "exact")
        if mode == "fast":
            # the first call of the opt-in mode on this scene: how many tiles it files for FP64 (the
            # context then switches to the FP64 pipeline by itself for the following calls)
            m.reset()
            dsm.process(rough, m, sync=True)
            gs = m.dsm_gather_stats()
        for _ in range(2):
            m.reset()
            dsm.process(rough, m, sync=False)
        m.synchronize()
        m.enable_timing(True)
        m.timing_reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(5):
            m.reset()
            dsm.process(rough, m, sync=False)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / 5
        m.synchronize()
        kt = m.kernel_times()
        m.enable_timing(False)
        e = {"dsm_ms_per_call": round(dt * 1e3, 3),
             "gather_ms": round(kt.get("k_dsm_gather", (0.0, 0))[0] / 5, 4)}
        if mode == "fast":
            e["note"] = ("the opt-in mode protects itself: a call that files more than half its tiles for "
                         "FP64 switches the context to the FP64 pipeline (sorted doubles) for the next 16 "
                         "calls; tiles_sent_to_fp64 is the first call's count, the timed calls ran after "
                         "the switch")
            e["tiles"] = gs["tiles"]
            e["tiles_sent_to_fp64"] = gs["f32_to_fp64"] + gs["f32_to_fp64_beyond"]
            e["tiles_sent_to_fp64_frac"] = round(e["tiles_sent_to_fp64"] / max(gs["tiles"], 1), 4)
            # (a download, not a device pointer: handing the pointer out would switch the layer
            # to eager refills for the rest of the run)
            elev_fast = torch.from_numpy(m.get("elevation"))
        else:
            d = (torch.from_numpy(m.get("elevation")) - elev_fast).abs()
            e["max_abs_diff_to_fast_mode_m"] = float(d[~torch.isnan(d)].max().item())
            e["nan_pattern_equal_to_fast_mode"] = bool(torch.equal(torch.isnan(d),
                                                                   torch.isnan(elev_fast)))
        res_out[mode] = e
    # the smooth cloud again in the run's own mode: the layers must not keep the rough scene
    m.set_dsm_precision(args.dsm_mode == "exact")
    del rough, elev_fast
    return res_out


def verify_windows(args, A, tiling, dist, one_gpu, dev, st, layout, rank, world, m, pts, settings,
                   exact=False):
    """Every window of the tiled run against ONE full-map DSM of the gathered cloud on rank 0
    (small workloads only).  Returns the comparison on rank 0, None elsewhere."""
    import numpy as np
    import torch
    elev = torch.from_numpy(m.get("elevation"))
    mine = (pts.cpu().contiguous(), elev)
    gathered = [None] * world
    dist.gather_object(mine, gathered if rank == 0 else None, dst=0)
    if rank != 0:
        return None
    cloud = torch.cat([g[0] for g in gathered], 0).to(dev)
    with A.AerialGridMap(st, device=dev.index) as full:
        full.set_dsm_precision(bool(exact) or args.dsm_mode == "exact")
        A.Dsm(settings, full).process(cloud, full)
        want = full.get("elevation")
    worst, nan_equal, cells = 0.0, True, 0
    for r in range(world):
        i0, j0, nr, nc = layout.window(r)
        got = gathered[r][1].numpy()
        ref = want[j0:j0 + nc, i0:i0 + nr]
        gn, wn = np.isnan(got), np.isnan(ref)
        nan_equal = nan_equal and bool(np.array_equal(gn, wn))
        ok = ~(gn | wn)
        if ok.any():
            worst = max(worst, float(np.abs(got[ok].astype(np.float64) - ref[ok]).max()))
        cells += int(got.size)
    return {"windows": world, "cells": cells, "nan_pattern_equal": nan_equal,
            "max_abs_err_m_vs_single_gpu": worst,
            "pass": bool(nan_equal and worst <= (1e-6 if exact else 1e-4))}


def preflight_verify(args, A, tiling, synth, dist, one_gpu, dev, local_rank, rank, world, stream,
                     tiles_i, tiles_j):
    """A small tiled DSM through the timed steps' own code path (TiledDsm over the process group,
    same window layout, every rank holding exactly the points of its own window -- generated the
    way the timed workload generates them) whose windows are gathered on rank 0 and compared with
    ONE single-GPU DSM of the gathered cloud: shows on the spot that the collective ran over
    `world` ranks and delivered the halo rows.  ~0.2 s; reported as `preflight` (a mismatch is
    reported, not fatal: the line then says that its numbers come from a broken exchange)."""
    import torch
    side, res, n_all = 2048, 0.25, 2_000_000
    layout = tiling.TileLayout(side, side, tiles_i, tiles_j)
    L = side * res
    st = A.GridMapSettings(0.0, 0.0, L, L, res)
    win = layout.window(rank)
    with A.AerialGridMap(st, device=local_rank, window=win) as pm:
        pm.set_stream(stream.cuda_stream)
        pm.set_dsm_precision(True)          # FP64: windows == full map but for the order of the sums
        center = (L / 2.0 - (win[0] + win[2] / 2.0) * res, L / 2.0 - (win[1] + win[3] / 2.0) * res)
        half = (win[2] * res / 2.0, win[3] * res / 2.0)
        pts = synth.make_points_torch(n_all // world, half, 900 + rank, dev, center=center)
        cx, cy = tiling.cell_coords(pts, pm.grid)
        kept = pts[tiling.owner_mask(cx, cy, win, layout)].contiguous()
        del pts, cx, cy
        n_own = int(kept.shape[0])
        wins_all = layout.windows()
        dens = max((n_all / world) / (w[2] * res * w[3] * res) for w in wins_all)
        edge = max(max(w[2], w[3]) * res for w in wins_all)
        cap = tiling.halo_strip_rows(dens, edge, 1, res)
        buf = torch.empty((n_own + tiling.MAX_DESTS * cap, 3), dtype=torch.float64, device=dev)
        buf[:n_own] = kept
        settings = A.DsmSettings(interpolation_radius=1)
        td = tiling.TiledDsm(settings, pm, layout, rank, cap,
                             comm=tiling.TorchComm(via_host=True) if one_gpu else None)
        pm.reset()
        td.process(buf, n_own, sync=True)
        v = verify_windows(args, A, tiling, dist, one_gpu, dev, st, layout, rank, world, pm, kept,
                           settings, exact=True)
    if rank != 0:
        return {"pass": True}
    v["neighbours_of_rank0"] = td.nbrs
    v["halo_rows_per_neighbour"] = cap
    v["map"] = "%dx%d cells, %d points, %d x %d windows" % (side, side, n_all, tiles_i, tiles_j)
    return v


def window_parity(map_, pts_dev, side, res, L, origin, exact, s=600):
    """Four s x s-cell windows of the resident elevation layer against the CPU oracle's DSM of the
    same cells (a grid of its own per window whose cell centres are the big map's: everything is
    dyadic, hence exact).  The big-cloud paths -- placement in rounds, clouds beyond 2^27 points --
    at full size, where a whole-map oracle run does not fit the host."""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_ffi as O
    which = "ref" if O.have_ref() else "port"
    s = min(s, side)
    wins = [(0, 0), ((side - s) // 2, (side - s) // 2), (side - s, side - s), (0, side - s)]
    elev = map_.as_torch("elevation")
    out = {"oracle": which, "window_cells": s * s, "windows": []}
    for i0, j0 in wins:
        sub_len = s * res
        cx = origin[0] + L / 2.0 - (i0 + s / 2.0) * res
        cy = origin[1] + L / 2.0 - (j0 + s / 2.0) * res
        g = O.make_grid(sub_len, sub_len, res, cx, cy, which=which)
        assert (g.rows, g.cols) == (s, s)
        halo = 3.0
        x, y = pts_dev[:, 0], pts_dev[:, 1]
        keep = (x > cx - sub_len / 2 - halo) & (x < cx + sub_len / 2 + halo) & \
               (y > cy - sub_len / 2 - halo) & (y < cy + sub_len / 2 + halo)
        sub = pts_dev[keep].cpu().numpy()
        rc, want, _ = O.dsm_process(sub, g, 1, 0.0, 0.0, which=which)
        assert rc == 0
        got = elev[j0:j0 + s, i0:i0 + s].cpu().numpy()
        ok = ~np.isnan(want)
        same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & ~ok)
        out["windows"].append({
            "cells": "[%d, %d) x [%d, %d)" % (i0, i0 + s, j0, j0 + s), "points": int(sub.shape[0]),
            "nan_pattern_equal": bool(np.array_equal(np.isnan(got), ~ok)),
            "max_abs_err_m": float(np.abs(got[ok].astype(np.float64) - want[ok]).max()) if ok.any() else 0.0,
            "bit_identical_frac": round(float(same.mean()), 9)})
    tol = 1e-6 if exact else 1e-4
    out["pass"] = all(w["nan_pattern_equal"] and w["max_abs_err_m"] <= tol for w in out["windows"])
    return out


def dump_outputs(out_dir, m, F, colored, rank, world):
    """--dump-outputs: the layers of the map as the last timed step left them, downloaded (not
    handed out as device pointers: that would change how the map refills them afterwards)."""
    import numpy as np
    names = ["elevation"]
    if F:
        names += ["elevation_angle", "num_observations", "observation_index",
                  "colored_ortho" if colored else "ortho"]
    os.makedirs(out_dir, exist_ok=True)
    buf = np.empty((m.cols, m.rows), np.float32)
    n = buf.size
    idx = None
    if n > DUMP_CELLS:
        rng = np.random.Generator(np.random.PCG64(DUMP_SEED))
        idx = np.sort(rng.choice(n, DUMP_CELLS, replace=False))
    prefix = "rank%d_" % rank if world > 1 else ""
    for name in names:
        m.get(name, out=buf)
        a = buf if idx is None else buf.reshape(-1)[idx]
        # (every file finite: NaN cells -- the reset value of elevation / observation_index /
        # colored_ortho where nothing was written -- become 0.0, and the mask says which they were)
        finite = np.isfinite(a)
        np.save(os.path.join(out_dir, prefix + name + ".npy"), np.where(finite, a, np.float32(0.0)))
        np.save(os.path.join(out_dir, prefix + name + "_finite.npy"), finite.astype(np.float32))


def other_workloads(args):
    """The other BASELINE configs on this GPU, each a CHILD `python bench.py --workload ...` of a few
    steps (its own process: its own contexts and memory, and nothing it does can cost the parent's
    line).  What DESIGN.md quotes beside the headline comes from here, keyed by the library's build."""
    import subprocess
    common = ["--steps", "5", "--warmup", "2", "--no-cpu-baseline", "--no-host-path", "--no-second-mode",
              "--no-rough-terrain", "--no-other-workloads", "--dsm-mode", args.dsm_mode]
    runs = [("cfg2 (configs[1]: DSM alone)", ["--workload", "cfg2"]),
            ("cfg2 --knn 4 (configs[1]'s optional 'IDW k = 4' cap: not a reference code path)",
             ["--workload", "cfg2", "--knn", "4"]),
            ("cfg3 --colored (8UC3 frames, colored_ortho)", ["--workload", "cfg3", "--colored"]),
            ("cfg4 at N = 1 (configs[3]'s whole 400M-point / 40000^2 map on one GPU)",
             ["--workload", "cfg4", "--window-parity"]),
            ("cfg5 at N = 1 (configs[4]: 64-frame batches onto the resident 40000^2 map)",
             ["--workload", "cfg5"])]
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    out = {}
    for name, extra in runs:
        t0 = time.perf_counter()
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__)] + common + extra, env=env,
                               stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True,
                               timeout=120)
            lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
            if not lines:
                out[name] = {"error": "child exit %d: %s" % (r.returncode, r.stderr[-300:])}
                continue
            d = json.loads(lines[-1])
            e = {"ms_per_step": d["ms_per_step"], "value": d["value"], "unit": d["unit"],
                 "library_build_id": d.get("library_build_id"),
                 "kernels_ms": {k: v.get("ms_per_step") for k, v in d.get("kernels", {}).items()},
                 "child_wall_s": round(time.perf_counter() - t0, 1)}
            if "window_parity" in d:
                e["window_parity"] = d["window_parity"]
            out[name] = e
        except subprocess.TimeoutExpired:
            # (one child that hangs is enough: the parent's own line must not wait for four more)
            out[name] = {"error": "did not finish in 120 s (killed); the remaining children were not started"}
            break
        except Exception as e:
            out[name] = {"error": repr(e)}
    return out


def session_route(args, A, st, tiles, devices, dsm_settings, ncam, mosaic_settings, h_pts, poses, h_frames,
                  cells_total, res, origin):
    """One pass of the whole map the way the C++ drop-in classes make it: cloud, frames and the
    GridMap's six matrices in (pageable) host memory, ONE amhip_session (one host process) over
    `devices` -- one window per device (AERIAL_MAPPER_HIP_DEVICES).  PCIe included."""
    import torch
    F = len(h_frames) if h_frames is not None else 0
    with A.HostSession(st, tiles=tiles, devices=devices) as hs:
        hs.set_dsm_precision(args.dsm_mode == "exact")
        for d in sorted(set(devices)):      # (loads the code objects on every device)
            warm = A.HostSession(A.GridMapSettings(origin[0], origin[1], 64 * res, 32 * res, res), devices=[d])
            warm.dsm_process(dsm_settings, h_pts[:4096])
            warm.close()
        for d in sorted(set(devices)):
            torch.cuda.synchronize(d)
        t0h = time.perf_counter()
        hs.dsm_process(dsm_settings, h_pts)
        dsm_s = time.perf_counter() - t0h
        prof = {"dsm": hs.last_profile()}        # (the read-outs are outside both timed calls)
        mosaic_s = 0.0
        if F:
            t1m = time.perf_counter()
            hs.ortho_process(ncam, mosaic_settings, poses, h_frames)
            mosaic_s = time.perf_counter() - t1m
            prof["mosaic"] = hs.last_profile()
        # a second pass over the SAME map (incremental mapping: the layers are resident,
        # the matrices unchanged since the session wrote them)
        t3h = time.perf_counter()
        hs.dsm_process(dsm_settings, h_pts)
        if F:
            hs.ortho_process(ncam, mosaic_settings, poses, h_frames)
        second_s = time.perf_counter() - t3h
        nwin = hs.num_windows
    bytes_up = h_pts.nbytes + (sum(f.nbytes for f in h_frames) * len(set(devices)) if F else 0)
    bytes_down = 4.0 * cells_total * (4 if F else 1)
    first_ms = (dsm_s + mosaic_s) * 1e3
    tot = lambda key: round(sum(c[key] for c in prof.values()), 3)
    return {"ms": round(first_ms, 1), "dsm_ms": round(dsm_s * 1e3, 1),
            "Mcells_per_s": round(cells_total / (first_ms * 1e-3) / 1e6, 1),
            # where the first pass went (amhip_session_last_profile, per call and summed): h2d = wall
            # clock until the call's inputs were handed to the copy engine (pageable sources block
            # that long), host_sum = host content sums (beside the upload: only their excess over
            # h2d is on the critical path), kernel / d2h = HIP events on the map's stream,
            # dev_sum_wait = device content sums that could not run beside a download
            "breakdown": {"h2d_ms": tot("h2d_ms"), "host_sum_ms": tot("host_sum_ms"),
                          "kernel_ms": tot("kernel_ms"), "dev_sum_wait_ms": tot("dev_sum_wait_ms"),
                          "d2h_ms": tot("d2h_ms"), "calls": prof},
            "second_pass_ms": round(second_s * 1e3, 1),
            "windows": nwin, "devices": [int(d) for d in devices],
            "bytes_up": bytes_up, "bytes_down": bytes_down,
            "link_floor_ms": round((bytes_up + bytes_down) / 56e9 / len(set(devices)) * 1e3, 1),
            "dsm_mode": args.dsm_mode,
            "note": "amhip_session_dsm_process + amhip_session_ortho_backward_process on pageable "
                    "host buffers (the drop-in classes' route, ONE host process): cloud (sliced over "
                    "the devices, routed device to device) + frames (replicated) up, the matrices "
                    "that changed down (elevation, elevation_angle, observation_index, ortho); "
                    "initial-state matrices are recognised by content and not uploaded; "
                    "link_floor_ms = those bytes at the 56 GB/s one device's link moves one way at a "
                    "time, the devices' links in parallel (H2D and D2H of one synchronous call "
                    "cannot overlap)"}


def session_route_all(args, A, synth, tiling, st, layout, world, one_gpu, dev, wl, fixed, pts_per_rank,
                      ox, oy, Lx, Ly, res, L, dsm_settings, ncam, mosaic_settings, F, ch, cells_total):
    """N > 1, rank 0 while the other ranks wait on the host: the WHOLE map (every rank's points,
    regenerated here with the ranks' seeds; every rank's frames) through one amhip_session with
    one window per device.  Skipped, with the reason, when the host lacks the memory."""
    import numpy as np
    import torch
    from aerial_mapper_amd import hip_lib
    try:
        import psutil
        avail = psutil.virtual_memory().available
    except Exception:
        avail = None
    need = 24.0 * pts_per_rank * world * 2 + 6 * 4.0 * cells_total * 1.2 + \
        (F * (1 if fixed else world) * wl["W"] * wl["H"] * ch * 2.0 if F else 0.0)
    if avail is not None and avail < 1.3 * need:
        if args.route == "session":
            raise SystemExit("--route session: the host has %.0f GB free, the whole map's host buffers "
                             "need %.0f GB" % (avail / 1e9, need / 1e9))
        return {"skipped": "host memory: %.0f GB free, %.0f GB needed for the whole map's matrices, "
                           "cloud and frames" % (avail / 1e9, need / 1e9)}
    try:
        parts, posel, framel = [], [], []
        for r in range(world):
            w = layout.window(r)
            center = (ox + Lx / 2.0 - (w[0] + w[2] / 2.0) * res, oy + Ly / 2.0 - (w[1] + w[3] / 2.0) * res)
            half = (w[2] * res / 2.0, w[3] * res / 2.0)
            p = synth.make_points_torch(pts_per_rank, half, 43 + r, dev, center=center)
            grid_full = hip_lib.make_grid(st.delta_easting, st.delta_northing, st.resolution,
                                            st.center_easting, st.center_northing)
            cx, cy = tiling.cell_coords(p, grid_full)
            parts.append(p[tiling.owner_mask(cx, cy, w, layout)].cpu().numpy())
            del p, cx, cy
            if F and (not fixed or r == 0):
                fl_center = (ox, oy) if fixed else center
                fr = synth.make_frames_torch(F, wl["H"], wl["W"], ch, 44 + (0 if fixed else r), dev)
                framel += [f for f in fr.cpu().numpy()]
                del fr
                posel.append(synth.make_lawnmower_poses(F, L / 2.0, wl["altitude"], 44 + (0 if fixed else r),
                                                        tilt_deg=5.0, center=fl_center))
        h_pts = np.concatenate(parts, 0)
        del parts
        devices = [0] * world if one_gpu else list(range(world))
        res_out = session_route(args, A, st, (layout.tiles_i, layout.tiles_j), devices, dsm_settings, ncam,
                                mosaic_settings if F else None, h_pts,
                                np.concatenate(posel, 0) if F else None, framel if F else None,
                                cells_total, res, (ox, oy))
        res_out["route"] = ("one host process, amhip_session over %d devices (AERIAL_MAPPER_HIP_DEVICES): what "
                            "an unchanged reference host gets; the line's `value` is the one-process-per-GPU "
                            "route with inputs resident in HBM" % len(set(devices)))
        res_out["points"] = int(h_pts.shape[0])
        res_out["frames"] = len(framel)
        return res_out
    except SystemExit:
        raise
    except Exception as e:   # the ranks' numbers stand on their own
        return {"error": repr(e)}


def valu_roofline(valu, dom, dom_ms, mode):
    """The VALU-issue roofline of the dominant kernel from the committed SQ counters of the same
    command in the same mode (lane-instructions per launch) over the LIVE kernel time."""
    prefixes = {"k_dsm_gather": ("k_dsm_gather_tiled<",) if mode == "exact" else ("k_dsm_gather_f32<",),
                "k_ortho_backward": ("k_ortho_backward",)}[dom]
    rows = [(k, v) for k, v in valu[1].items() if k.startswith(prefixes) and v.get("GRBM_GUI_ACTIVE")]
    if not rows:
        return {}
    kname, v = max(rows, key=lambda r: r[1].get("SQ_INSTS_VALU", 0))
    busy = v["GRBM_GUI_ACTIVE"] / 8.0           # summed over the 8 XCDs
    lanes = v.get("SQ_THREAD_CYCLES_VALU", 0.0) / max(v["SQ_INSTS_VALU"], 1.0) / 64.0
    # 256 CUs x 4 SIMDs x 32 lanes x 2.4 GHz = 78.6 T lane-instructions/s (one f32 op per lane
    # and cycle; FP64 ops issue at half that: a pure FP64 stream tops out at frac 0.5)
    peak_valu = 256 * 4 * 32 * 2.4e9
    lane_ops = v["SQ_INSTS_VALU"] * 64.0 * lanes
    fp64 = mode == "exact" or dom == "k_ortho_backward"
    # (`bound` stays "hbm" -- the roofline north_star mandates and `achieved` / `peak` / `frac` are quoted on;
    # what actually limits the kernel is said beside it)
    return {"limited_by": ("valu (FP64 issue), not HBM" if fp64 else "valu (f32 + FP64 issue), not HBM"), "valu": {
        "kernel": kname,
        "note": ("FP64 VALU-issue bound (every pair's test and weight in the reference's doubles: "
                 "v_*_f64 issue at half rate, 4.4 cycles per wave-instruction measured), not HBM "
                 "bound; no MFMA-shaped work on this path" if fp64 else
                 "VALU-issue bound (f32 pair arithmetic + FP64 staging / decisions), not HBM bound; "
                 "no MFMA-shaped work on this path"),
        "frac": round(lane_ops / (dom_ms * 1e-3) / peak_valu, 4),
        "frac_ceiling_for_this_instruction_mix": 0.5 if fp64 else 0.65,
        "lane_instructions_per_launch": lane_ops, "peak_lane_instructions_per_s": peak_valu,
        # wave-instructions per SIMD and clock.  What one costs, measured in real shader cycles
        # (s_memtime; tools/ubench/ubench3.hip, profiles/r03_ubench3_real_cycles.jsonl)
        "wave_instructions_per_simd_clock": round(v["SQ_INSTS_VALU"] / 1024.0 / busy, 3),
        "issue_cycles_per_wave_instruction_measured": {
            "full_rate (v_fma/mul/add_f32, v_sub_u32)": 2.4,
            "half_rate (v_cvt_f32_i32, v_cmp/cmpx_f32, v_max_f32, FP64 fma/mul/add)": 4.4,
            "v_rcp_f32": 8.2, "source": "profiles/r03_ubench3_real_cycles.jsonl"},
        "lanes_active_frac": round(lanes, 3),
        "source": valu[0] + " (counters of the same command in the same mode); kernel_ms live"}}


def main():
    args = parse()
    import numpy as np
    import torch

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no HIP device visible); there is no CPU fallback")
    if args.session_child:
        args.gpus = args.session_child
        os.environ["WORLD_SIZE"] = str(args.session_child)   # (geometry only: no process group is made)
        os.environ["RANK"] = os.environ["LOCAL_RANK"] = "0"
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` without a launcher: start the N ranks ourselves (one process
        # per GPU over RCCL) instead of silently timing one.  The reference host is ONE process
        # (main-dsm.cc:103-107); its own multi-device route is timed by --route session.
        have = torch.cuda.device_count()
        if have < args.gpus and os.environ.get("AMHIP_BENCH_ONE_GPU", "0") != "1":
            raise SystemExit("bench.py --gpus %d: only %d HIP device(s) visible; refusing to print a line "
                             "for fewer GPUs than asked (AMHIP_BENCH_ONE_GPU=1 rehearses the N-rank "
                             "path on one device, labelled as such)" % (args.gpus, have))
        import socket
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
               "--nproc-per-node", str(args.gpus), "--master-addr", "127.0.0.1",
               "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        sys.stdout.flush()
        # a CHILD process, never exec: this process has already initialised the GPU (device_count),
        # and replacing the program of such a process is not safe on every driver
        import subprocess
        raise SystemExit(subprocess.call(cmd))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if args.gpus != world:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d: refusing to print a line whose n_gpus differs "
                         "from what was asked" % (args.gpus, world))
    # AMHIP_BENCH_ONE_GPU=1: rehearsal of the N > 1 code path on a 1-GPU box -- every rank
    # on device 0, gloo instead of RCCL (which refuses two ranks per device), the halo rows
    # staged through host memory.  Its numbers mean nothing; the line says so.
    one_gpu = world > 1 and os.environ.get("AMHIP_BENCH_ONE_GPU", "0") == "1"
    if one_gpu:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    # ONE explicit HIP stream for everything in the timed region: torch's
    # generators, the library's kernels (amhip_ctx_set_stream), the per-kernel
    # HIP events and -- for N > 1 -- the RCCL all_to_all are all ordered on it.
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(stream)
    dist = host_pg = None
    if world > 1 and not args.session_child:
        import torch.distributed as dist
        if one_gpu:
            dist.init_process_group("gloo")
            host_pg = None
        else:
            dist.init_process_group("nccl", device_id=dev)
            # a host-side group for the LAST wait: while rank 0 drives every device through one
            # amhip_session (session_route) the other ranks must not spin in an RCCL kernel
            host_pg = dist.new_group(backend="gloo")

    import aerial_mapper_amd as A
    from aerial_mapper_amd import synth

    from aerial_mapper_amd import tiling
    wl = WORKLOADS[args.workload]
    side, res = wl["side"], wl["res"]
    L = side * res
    ox, oy = (float(v) for v in args.map_origin.split(","))
    fixed = bool(wl.get("fixed_map"))
    if fixed:
        # ONE fixed survey (strong scaling): the map is cut into windows, 2 x 4 on a node's 8 GPUs
        Lx = Ly = L
        rows_all = cols_all = side
        layout = (tiling.TileLayout(side, side, 2, 4) if world == 8
                  else tiling.TileLayout.for_world(side, side, world))
        pts_per_rank = wl["points"] // world
    else:
        # ONE survey map of world x 1 tiles (weak scaling: every rank owns a side x side window
        # of it, cell positions are those of the full map)
        Lx, Ly = world * L, L
        rows_all, cols_all = world * side, side
        layout = tiling.TileLayout(rows_all, cols_all, world, 1)
        pts_per_rank = wl["points"]
    st = A.GridMapSettings(ox, oy, Lx, Ly, res)
    if args.session_child:
        # (internal) the whole map of an N-rank run through ONE amhip_session with one window per
        # device: prints the `session_route` object and nothing else
        # (tests/test_gpu_bench_multirank.py: AMHIP_BENCH_SESSION_CHILD_FAULT=exit | hang rehearses the
        # parent's two failure paths -- the ranks' line must be printed either way)
        fault = os.environ.get("AMHIP_BENCH_SESSION_CHILD_FAULT")
        if fault == "exit":
            raise SystemExit("session child: injected failure")
        if fault == "hang":
            time.sleep(3600)
        F = wl["frames"]
        ch = 3 if args.colored else 1
        ncam = A.NCamera(wl["f"], wl["f"], (wl["W"] - 1) / 2.0, (wl["H"] - 1) / 2.0, wl["W"], wl["H"]) if F else None
        res_out = session_route_all(args, A, synth, tiling, st, layout, world, one_gpu, dev, wl, fixed,
                                    pts_per_rank, ox, oy, Lx, Ly, res, L, A.DsmSettings(interpolation_radius=1),
                                    ncam, A.OrthoSettings(colored_ortho=args.colored), F, ch,
                                    rows_all * cols_all)
        print(json.dumps(res_out))
        return
    win = layout.window(rank)
    m = A.AerialGridMap(st, device=local_rank, window=win)
    m.set_stream(stream.cuda_stream)
    if args.knn:
        m.set_dsm_knn(args.knn)
    # the gather's arithmetic in the timed steps (the library's own default is EXACT since round 3)
    m.set_dsm_precision(args.dsm_mode == "exact")
    # centre of this rank's window in map coordinates (x decreases with i, y with j)
    tile_center = (ox + Lx / 2.0 - (win[0] + win[2] / 2.0) * res,
                   oy + Ly / 2.0 - (win[1] + win[3] / 2.0) * res)
    win_lx, win_ly = win[2] * res, win[3] * res

    # inputs, generated in HBM (synthetic, seeded).  N = 1: the map's points plus a 4 m apron.
    # N > 1: each rank holds exactly the points of ITS window; the halo strips are exchanged
    # with the neighbouring windows over RCCL inside every step (tiling.TiledDsm).
    apron = 4.0 if world == 1 else 0.0
    n_pts = pts_per_rank
    halo_cap = 0       # rows per (source, destination) pair of the halo exchange
    if world > 1:
        # (the same on every rank -- it is a split size of the all_to_all: densest window, longest edge)
        wins_all = layout.windows()
        dens = max(pts_per_rank / (w[2] * res * w[3] * res) for w in wins_all)
        edge = max(max(w[2], w[3]) * res for w in wins_all)
        halo_cap = tiling.halo_strip_rows(dens, edge, 1, res)
    pts_buf = torch.empty((n_pts + tiling.MAX_DESTS * halo_cap, 3), dtype=torch.float64, device=dev)
    # (N > 1: window edges are multiples of 64 cells, so a window is not exactly L wide;
    # its points cover exactly its own extent, no strip of the map is left without points)
    half = (win_lx / 2.0 + apron, win_ly / 2.0 + apron)
    if wl.get("mt19937_seed") is not None:
        if world != 1 or (ox, oy) != (0.0, 0.0):
            raise SystemExit("--workload %s is a fixed single-GPU input (BASELINE.json configs[0])" % args.workload)
        pts_buf[:n_pts] = torch.from_numpy(synth.make_points_cfg1(n_pts, L / 2.0, wl["mt19937_seed"])).to(dev)
    else:
        pts_buf[:n_pts] = synth.make_points_torch(n_pts, half, 43 + rank, dev, center=tile_center)
    if world > 1:
        # keep only points whose cell is inside the window (a point exactly on
        # the upper edge belongs to the neighbour)
        cxx, cyy = tiling.cell_coords(pts_buf[:n_pts], m.grid)
        own = tiling.owner_mask(cxx, cyy, win, layout)
        kept = pts_buf[:n_pts][own]
        n_pts = int(kept.shape[0])
        pts_buf[:n_pts] = kept
        del cxx, cyy, own, kept
    pts = pts_buf[:n_pts]
    F = wl["frames"]
    batch = wl.get("batch", 0)
    ch = 3 if args.colored else 1
    frames = poses = ncam = mosaic = None
    if F:
        # (cfg5: the frames of the WHOLE flight over the whole map, replicated on every rank)
        fl_center = (ox, oy) if fixed else tile_center
        frames = synth.make_frames_torch(F, wl["H"], wl["W"], ch, 44 + (0 if fixed else rank), dev)
        poses = synth.make_lawnmower_poses(F, L / 2.0, wl["altitude"], 44 + (0 if fixed else rank),
                                           tilt_deg=5.0, center=fl_center)
        ncam = A.NCamera(wl["f"], wl["f"], (wl["W"] - 1) / 2.0, (wl["H"] - 1) / 2.0,
                         wl["W"], wl["H"])
        mosaic = A.OrthoBackwardGrid(ncam, A.OrthoSettings(colored_ortho=args.colored), m)
    dsm = A.Dsm(A.DsmSettings(interpolation_radius=1), m)

    tiled = None
    if world > 1:
        # the DSM's binning pass selects the halo points on its way, one all_to_all (rows only
        # between geometric neighbours) ships them, nothing synchronises with the host in a step
        tiled = tiling.TiledDsm(dsm.settings, m, layout, rank, halo_cap,
                                comm=tiling.TorchComm(via_host=True) if one_gpu else None)

    def run_dsm():
        if tiled is not None:
            tiled.process(pts_buf, n_pts, sync=False)
        else:
            dsm.process(pts, m, sync=False)

    if batch:
        # incremental mapping: layers stay resident, every step appends the next batch
        m.reset()
        run_dsm()
        m.synchronize()
        nb = (F + batch - 1) // batch
        state = {"b": 0}

        def step():
            b = state["b"] % nb
            state["b"] += 1
            lo, hi = b * batch, min((b + 1) * batch, F)
            mosaic.process(poses[lo:hi], frames[lo:hi], m, sync=False)
    else:
        def step():
            m.reset()
            run_dsm()
            if F:
                mosaic.process(poses, frames, m, sync=False)

    def fence():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
            torch.cuda.synchronize()

    # ---- N > 1: who is here, and does the exchange deliver?  (self-proving first run) ----------
    ranks_info = preflight = None
    if dist is not None:
        props = torch.cuda.get_device_properties(dev)
        mine = {"rank": rank, "local_rank": local_rank, "device_index": dev.index,
                "device_name": props.name, "pci_bus_id": getattr(props, "pci_bus_id", None),
                "uuid": str(getattr(props, "uuid", "")), "host": os.uname().nodename,
                "visible": os.environ.get("HIP_VISIBLE_DEVICES", os.environ.get("ROCR_VISIBLE_DEVICES"))}
        gathered = [None] * world
        dist.all_gather_object(gathered, mine)
        ranks_info = {"backend": dist.get_backend(), "world_size_reported": dist.get_world_size(),
                      "ranks": gathered,
                      "distinct_devices": len(set((g["host"], g["device_index"], g["uuid"]) for g in gathered))}
        if args.full and not args.no_preflight:
            preflight = preflight_verify(args, A, tiling, synth, dist, one_gpu, dev, local_rank, rank,
                                         world, stream, layout.tiles_i, layout.tiles_j)
            if rank == 0 and not preflight["pass"]:
                sys.stderr.write("bench.py: PREFLIGHT FAILED -- the tiled DSM does not reproduce the "
                                 "single-GPU result: %s\n" % json.dumps(preflight))

    for _ in range(args.warmup):
        step()
    m.synchronize()  # also surfaces device-side CHECK failures
    m.enable_timing(True)
    m.timing_reset()
    fence()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    fence()
    dt = time.perf_counter() - t0
    m.synchronize()
    if dist is not None:
        tmax = torch.tensor([dt], dtype=torch.float64, device="cpu" if one_gpu else dev)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        dt = float(tmax.item())
    ktimes = m.kernel_times()
    m.enable_timing(False)
    if tiled is not None:
        tiled.check_overflow()
    if args.dump_outputs:
        # (before anything else runs: the layers still hold the result of the last timed step)
        dump_outputs(args.dump_outputs, m, F, args.colored, rank, world)
    verify = None
    if args.verify and world > 1:
        verify = verify_windows(args, A, tiling, dist, one_gpu, dev, st, layout, rank, world, m, pts,
                                dsm.settings)

    def timed_loop(nsteps, nwarm):
        """(N = 1 extras) nwarm + nsteps more steps with the current settings -> (s per step, kernel ms)"""
        for _ in range(nwarm):
            step()
        m.synchronize()
        m.enable_timing(True)
        m.timing_reset()
        torch.cuda.synchronize()
        t0x = time.perf_counter()
        for _ in range(nsteps):
            step()
        torch.cuda.synchronize()
        dtx = time.perf_counter() - t0x
        m.synchronize()
        kt = m.kernel_times()
        m.enable_timing(False)
        return dtx / nsteps, {k: v[0] / nsteps for k, v in kt.items() if v[1]}

    cells = win[2] * win[3] if not fixed else side * side // world   # per rank (reported)
    cells_all = rows_all * cols_all
    value = cells_all * args.steps / dt / 1e6

    if rank == 0:
        N = pts_per_rank
        if batch:
            F_step = batch
            b_dsm = 0.0
        else:
            F_step = F
            b_dsm = 24.0 * N + 4.0 * cells
        b_ortho = (20.0 * cells + F_step * wl["W"] * wl["H"] * ch + 56.0 * F_step) if F else 0.0
        alg_bytes = {"k_dsm_gather": b_dsm, "k_ortho_backward": b_ortho}
        # PMC evidence of the same command IN THE SAME ARITHMETIC MODE, collected by
        # tools/collect_profiles.sh and committed under profiles/ (newest round first; the file
        # name and a "dsm_mode" key inside both carry the mode, so the other mode's counters can
        # never be picked); never measured inside this run -- the line says so
        import glob
        import re

        def newest(pattern):
            fs = glob.glob(os.path.join(ROOT, "profiles", pattern))
            def key(f):
                mm = re.search(r"r(\d+)_", os.path.basename(f))
                return int(mm.group(1)) if mm else 0
            return sorted(fs, key=key)[-1] if fs else None

        from aerial_mapper_amd import hip_lib
        lib_build = hip_lib.build_id()
        stale = {}

        def evidence(mode):
            """(traffic per slot, its file, SQ counters per kernel, their file) of `mode` -- only from
            summaries collected from THIS build of the library (amhip_build_id; VERDICT r4 weak #5: a
            kernel change without a new tools/collect_profiles.sh run must not leave old counters in
            the line)"""
            tr, tr_src, sq, sq_src = {}, None, None, None
            try:
                f = newest("r*_%s_pmc_traffic.json" % mode)
                tj = json.load(open(f))
                if tj.get("workload") == args.workload and tj.get("dsm_mode") == mode and not args.colored:
                    if tj.get("build_id") == lib_build:
                        tr = {k: v["bytes"] for k, v in tj["kernels"].items()}
                        tr_src = "profiles/" + os.path.basename(f)
                    else:
                        stale[mode] = ("profiles/%s was collected from build %s, the library is build %s: "
                                       "not used" % (os.path.basename(f), tj.get("build_id"), lib_build))
            except Exception:
                pass
            try:
                f = newest("r*_%s_cfg3_pmc_sq.json" % mode)
                sj = json.load(open(f)) if f else {}
                if f and sj.get("dsm_mode") == mode and args.workload in ("cfg3", "cfg2") and not args.colored \
                        and sj.get("build_id") == lib_build:
                    sq, sq_src = sj["kernels"], "profiles/" + os.path.basename(f)
            except Exception:
                pass
            return tr, tr_src, sq, sq_src

        traffic, traffic_src, valu_k, valu_src = evidence(args.dsm_mode)
        valu = (valu_src, valu_k) if valu_k else None
        kern = {}
        for name, (ms, n) in ktimes.items():
            if n:
                per_step = ms / args.steps
                kern[name] = {"ms_per_step": round(per_step, 4), "launches_per_step": n / args.steps}
        dom = max((k for k in kern if k in alg_bytes and alg_bytes[k] > 0),
                  key=lambda k: kern[k]["ms_per_step"])
        dom_ms = kern[dom]["ms_per_step"] / kern[dom]["launches_per_step"]
        achieved = alg_bytes[dom] / (dom_ms * 1e-3) / 1e9
        total_alg = b_dsm + b_ortho
        out = {
            "metric": ("Mcells/s (DSM+ortho)" if F else "Mcells/s (DSM)") +
                      (" [OPTIONAL k=%d capped mode: not the reference's algorithm]" % args.knn if args.knn else ""),
            "value": round(value, 2), "unit": "Mcells/s", "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(dt / args.steps * 1e3, 3),
            "higher_is_better": True, "scaling": "strong" if fixed else "weak", "vs_baseline": None,
            "dtype": "f64 (decisions, staging, mosaic) + f32 (DSM pair arithmetic under exact guards)"
            if args.dsm_mode == "fast" else "f64", "data": "synthetic" if not one_gpu else
            "synthetic; REHEARSAL: %d ranks on one GPU over gloo, not a measurement" % world,
            "config": {"workload": args.workload + ": " + (wl["desc"].replace("8UC1", "8UC3 (colored_ortho)")
                                                          if args.colored else wl["desc"]),
                       "dsm_mode": {"fast": "AMHIP_DSM_FAST (opt-in: single precision under exact guards, "
                                            "heights within the north_star's 1e-4 m; the library's "
                                            "default mode is timed beside it: exact_mode)",
                                    "exact": "AMHIP_DSM_EXACT (the library's default: FP64, the "
                                             "reference's arithmetic and floats; the opt-in single-"
                                             "precision mode is timed beside it: fast_mode)"}[args.dsm_mode],
                       "sort_pipeline": "counting sort on every call (count, two scatter passes, placement); "
                                        "the same pipeline at every N (a tiled call's count pass also "
                                        "selects the halo)",
                       "cells_per_gpu": cells, "points_per_gpu": N, "frames": F_step,
                       "step": "layers reset (lazy: the fills are fused into the kernels that "
                               "produce the layers; AMHIP_TUNING=eager_reset for plain fills) + "
                               "%sDsm::process + OrthoBackwardGrid::process, inputs resident in HBM" %
                               ("halo exchange (RCCL all_to_all) + " if world > 1 else ""),
                       "parallelism": "one map, %d x %d windows, one per GPU" % (layout.tiles_i, layout.tiles_j)},
            # the contract's HBM roofline of the dominant kernel (algorithmic bytes / live
            # HIP-event time / 8 TB/s) -- and, because nothing on this path is HBM bound, what
            # does bound it (below: "bound", "valu")
            "roofline": {"bound": "hbm", "kernel": dom, "achieved": round(achieved, 1),
                         "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": round(achieved / HBM_PEAK_GBS, 4),
                         "traffic": traffic.get(dom), "traffic_source": traffic_src,
                         "algorithmic_bytes_per_launch": alg_bytes[dom],
                         "kernel_ms": round(dom_ms, 4)},
            "whole_step_hbm": {"algorithmic_bytes": total_alg,
                               "achieved_GBs": round(total_alg / (dt / args.steps) / 1e9, 1),
                               "frac": round(total_alg / (dt / args.steps) / 1e9 / HBM_PEAK_GBS, 4)},
            "kernels": kern,
            "dsm_stats": m.dsm_stats(),
            "library_build_id": lib_build,
        }
        if stale.get(args.dsm_mode):
            out["roofline"]["traffic_stale"] = stale[args.dsm_mode]
        # counter traffic can only be >= what the kernel must move: a smaller figure is a broken
        # summary (round 2: every entry halved), refused rather than printed
        tr = out["roofline"]["traffic"]
        # (single-precision mode since round 3: the sort hands the gather 16-byte records -- fixed-
        # point position + f32 height offset -- instead of the 24-byte points the algorithmic figure
        # counts, so that kernel's floor is 16 N + 4 C; the FP64 mode's is the algorithmic figure)
        must_move = dict(alg_bytes)
        if dom == "k_dsm_gather" and args.dsm_mode == "fast" and not batch:
            must_move[dom] = 16.0 * N + 4.0 * cells
            out["roofline"]["kernel_reads_records"] = ("16-byte sort records (amhip_sort.hip make_record), not the "
                                                       "24-byte points of algorithmic_bytes_per_launch: the "
                                                       "kernel's own floor is %d B" % int(must_move[dom]))
        if tr is not None:
            if tr < 0.9 * must_move[dom]:
                out["roofline"]["traffic"] = None
                out["roofline"]["traffic_rejected"] = ("%s reports %d B for %s, below 0.9 x the %d B the kernel "
                                                       "must move: not credible" % (traffic_src, tr, dom, int(must_move[dom])))
            else:
                out["roofline"]["traffic_over_algorithmic"] = round(tr / alg_bytes[dom], 3)
        if traffic:
            step_traffic = float(sum(traffic.values()))
            if step_traffic >= 0.9 * total_alg:
                out["whole_step_hbm"]["traffic"] = int(step_traffic)
                out["whole_step_hbm"]["traffic_over_algorithmic"] = round(step_traffic / total_alg, 3)
                out["whole_step_hbm"]["traffic_source"] = traffic_src
        if ranks_info is not None:
            out["ranks"] = ranks_info
        if preflight is not None:
            out["preflight"] = preflight
        if world == 1:
            out["path"] = "single context (no collective): the N = 1 point of the scaling sweep is this line"
        if batch:
            out["config"]["step"] = ("OrthoBackwardGrid::process of one %d-frame batch onto the resident "
                                     "layers (the DSM was built once before the timed steps)" % batch)
        if verify is not None:
            out["verify"] = verify
        if valu is not None:
            out["roofline"].update(valu_roofline(valu, dom, dom_ms, args.dsm_mode))
        parity_done = False
        if world == 1 and args.full and not args.no_cpu_baseline and not fixed:
            # (before anything else runs: the layers still hold the result of the TIMED steps)
            refs = None
            try:
                refs, cb = cpu_baseline(args, wl, m, pts, frames, poses, ncam, tile_center)
                parity = parity_against(refs, args, m, poses, ncam, F)
                parity["pass"] = "timed"
                parity["dsm_mode"] = args.dsm_mode
                out["cpu_baseline"] = cb
                out["parity_sample"] = parity
            except Exception as e:  # the GPU number stands on its own
                out["cpu_baseline"] = {"error": repr(e)}
            parity_done = True
            if not args.no_second_mode and not args.knn:
                # the OTHER arithmetic mode, driver-timed in the same run
                other = "exact" if args.dsm_mode == "fast" else "fast"
                m.set_dsm_precision(other == "exact")
                k2 = max(3, min(args.steps, 10))
                sec, kms = timed_loop(k2, 2)
                om = {"dsm_mode": other, "steps": k2, "ms_per_step": round(sec * 1e3, 3),
                      "Mcells_per_s": round(cells_all / sec / 1e6, 1),
                      "gather_ms": round(kms.get("k_dsm_gather", 0.0), 4),
                      "kernels_ms": {k: round(v, 4) for k, v in kms.items()}}
                if refs is not None:
                    try:
                        om["parity_sample"] = parity_against(refs, args, m, poses, ncam, F)
                    except Exception as e:
                        om["parity_sample"] = {"error": repr(e)}
                # the same roofline object for this mode's gather, from ITS committed counters
                if om["gather_ms"] > 0 and b_dsm > 0:
                    o_tr, o_src, o_sq, o_sq_src = evidence(other)
                    o_ach = b_dsm / (om["gather_ms"] * 1e-3) / 1e9
                    orl = {"bound": "hbm", "kernel": "k_dsm_gather", "achieved": round(o_ach, 1),
                           "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(o_ach / HBM_PEAK_GBS, 4),
                           "traffic": o_tr.get("k_dsm_gather"), "traffic_source": o_src,
                           "algorithmic_bytes_per_launch": b_dsm, "kernel_ms": om["gather_ms"]}
                    if orl["traffic"]:
                        orl["traffic_over_algorithmic"] = round(orl["traffic"] / b_dsm, 3)
                    if o_sq:
                        orl.update(valu_roofline((o_sq_src, o_sq), "k_dsm_gather", om["gather_ms"], other))
                    om["roofline"] = orl
                out[other + "_mode"] = om
                m.set_dsm_precision(args.dsm_mode == "exact")
                # what a host that never touches the switch gets for the byte-exact half
                dflt = out.get("exact_mode", {}).get("parity_sample") if args.dsm_mode == "fast" \
                    else out.get("parity_sample")
                if dflt and F:
                    key = ("colored_ortho" if args.colored else "ortho") + "_mismatch_cells"
                    out["ortho_mismatch_cells_default_mode"] = dflt.get(key)
                    out["ortho_mismatch_cells_fast_mode"] = (
                        out["parity_sample"] if args.dsm_mode == "fast" else om.get("parity_sample", {})).get(key)
            del refs
        # The launch policy a repeated call takes from its predecessor: kernels whose work
        # lists were empty last time are not launched.  The same steps with every one launched = what
        # a context's very first call runs.
        if world == 1 and args.full and not batch and not args.knn and tiled is None:
            try:
                from aerial_mapper_amd import hip_lib as _hl
                k3 = max(3, min(args.steps, 10))
                _hl.set_tuning("no_launch_skips", 1)
                try:
                    sec, kms = timed_loop(k3, 1)
                    m.synchronize()
                finally:
                    _hl.set_tuning("no_launch_skips", None)
                out["launch_skips"] = {
                    "value_uses": "the library's default: empty class / big-list kernels of the previous "
                                  "call's geometry are not launched",
                    "all_launched": {"steps": k3, "ms_per_step": round(sec * 1e3, 3),
                                     "Mcells_per_s": round(cells_all / sec / 1e6, 1)},
                    "gain_ms": round(sec * 1e3 - out["ms_per_step"], 3)}
                timed_loop(1, 0)
            except Exception as e:
                out["launch_skips"] = {"error": repr(e)}
        if world == 1 and args.full and not fixed and not args.no_rough_terrain and not args.knn and not batch \
                and not wl.get("mt19937_seed"):
            try:
                out["rough_terrain"] = rough_terrain(args, A, m, pts, dsm, side, res, tile_center, L)
            except Exception as e:
                out["rough_terrain"] = {"error": repr(e)}
        if world == 1 and fixed and args.window_parity and not args.knn:
            try:
                out["window_parity"] = window_parity(m, pts, side, res, L, (ox, oy), args.dsm_mode == "exact")
            except Exception as e:
                out["window_parity"] = {"error": repr(e)}
        # (the host-buffer route: with --full, or when --route session asks for it by name)
        host_route = args.route == "session" or (args.full and args.route == "auto")
        if world == 1 and args.host_path and not fixed and host_route:
            h_pts = pts.cpu().numpy()
            h_frames = [f for f in frames.cpu().numpy()] if F else None
            out["pcie_inclusive"] = session_route(args, A, st, (1, 1), [local_rank], dsm.settings, ncam,
                                                  mosaic.settings if F else None, h_pts, poses, h_frames,
                                                  cells, res, (ox, oy))
            out["pcie_inclusive"]["route"] = "session (--route session at N = 1 is this object)"
        if world == 1 and args.full and args.workload == "cfg3" and not args.no_other_workloads and not args.knn \
                and not args.colored and not args.no_cpu_baseline:
            # (after everything of this process: the children need the GPU's memory -- cfg4 / cfg5 hold
            # a 40000^2 map -- so this process's buffers go first)
            try:
                del frames, pts, pts_buf
                m.close()
                torch.cuda.empty_cache()
            except Exception:
                pass
            out["other_workloads"] = other_workloads(args)
        if world > 1 and host_route and not batch:
            # In a CHILD process with a time limit: one host process driving all N devices has never
            # run next to N live ranks on real hardware -- whatever it does (fail, hang), this
            # line's own numbers are already measured and must be printed.  The ranks wait on the
            # host meanwhile (gloo), not in an RCCL kernel.
            import subprocess
            cmd = [sys.executable, os.path.abspath(__file__), "--session-child", str(world), "--workload",
                   args.workload, "--dsm-mode", args.dsm_mode, "--route", args.route, "--map-origin",
                   args.map_origin] + (["--colored"] if args.colored else [])
            env = dict(os.environ)
            for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "GROUP_RANK", "ROLE_RANK",
                      "TORCHELASTIC_RUN_ID", "MASTER_PORT"):
                env.pop(k, None)
            limit = float(os.environ.get("AMHIP_BENCH_SESSION_TIMEOUT", "180"))
            try:
                r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                                   universal_newlines=True, timeout=limit)
                lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
                out["session_route"] = json.loads(lines[-1]) if lines else {
                    "error": "child exit %d: %s" % (r.returncode, r.stderr[-400:])}
            except subprocess.TimeoutExpired:
                out["session_route"] = {"error": "the one-process session over %d devices did not finish in "
                                                 "%.0f s (killed); the ranks' numbers above are unaffected"
                                                 % (world, limit)}
            except Exception as e:
                out["session_route"] = {"error": repr(e)}
        print(json.dumps(out))
        sys.stdout.flush()
    if dist is not None:
        dist.barrier(group=host_pg) if host_pg is not None else dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
