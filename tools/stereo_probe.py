"""One JSON line: ms of rectify, the block matcher (the k_stereo slot), densify and DSM for a 1920x1080
stereo pair with the reference's parameters of that matcher (BlockMatchingParameters::SGBM, or ::BM
with --matcher bm), median of --reps runs after a warm-up, plus the library's build id.
Usage: python tools/stereo_probe.py [--reps N] [--matcher {sgbm,bm}]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--matcher", choices=("sgbm", "bm"), default="sgbm")
    args = ap.parse_args()
    import numpy as np
    import torch
    import aerial_mapper_amd as A
    from aerial_mapper_amd import hip_lib
    from test_oracle_rectify import rig
    W, H = 1920, 1080
    K, R1, R2, t1, t2, left, right = rig(21, W=W, H=H)
    lt, rt = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
    out = {}
    name = args.matcher
    if name == "bm":
        params = A.BmParameters()
        match = A.compute_disparity_bm
    else:
        params = A.SgbmParameters()
        match = A.compute_disparity_sgbm
    with A.AerialGridMap(A.GridMapSettings(12.0, -4.0, 400.0, 300.0, 0.5)) as m:
        dsm = A.Dsm(A.DsmSettings(1), m)
        runs = []
        for rep in range(args.reps + 1):
            ms = {}
            t0 = time.perf_counter()
            r = A.rectify_stereo_pair(m, K, R1, R2, t1, t2, lt, rt)
            ms["rectify"] = (time.perf_counter() - t0) * 1e3
            m.enable_timing(True)
            m.timing_reset()
            t0 = time.perf_counter()
            disp = match(m, r["image_left"], r["image_right"], params, mask=r["mask"])
            ms[name + "_wall"] = (time.perf_counter() - t0) * 1e3
            ms[name] = m.kernel_times()["k_stereo"][0]
            m.enable_timing(False)
            t0 = time.perf_counter()
            pts, inten = A.densify(m, disp, r["image_left"], K, r["baseline"], r["R_G_C"], t1)
            ms["densify"] = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            dsm.process(pts, m)
            m.synchronize()
            ms["dsm"] = (time.perf_counter() - t0) * 1e3
            ms["points"] = int(pts.shape[0])
            if rep:
                runs.append(ms)
        for k in runs[0]:
            out[k] = float(np.median([r[k] for r in runs])) if k != "points" else runs[0][k]
    out.update({"width": W, "height": H, "num_disparities": params.num_disparities,
                "block_size": params.block_size, "reps": args.reps, "build_id": hip_lib.build_id(),
                "note": "rectify / densify / dsm: wall ms of the synchronous Python calls; %s: "
                        "HIP-event ms of the k_stereo slot (%s_wall: the call's wall time)" % (name, name)})
    if name == "bm":
        out["matcher"] = "bm"
    print(json.dumps(out))


if __name__ == "__main__":
    main()
