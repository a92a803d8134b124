"""One JSON line: wall-clock ms of a whole frame sequence -> one dense cloud, F = 9 frames of
1920x1080 from tests/stereo_sequence.py's generator, for BM and SGBM, three ways:
  (a) pair_loop    a Python loop of dense_cloud_from_stereo_pair over the 8 pairs, frames already
                   on the device (what there was before stereo::Stereo: a synchronisation, a count
                   read-back and worst-case allocations per step of every pair);
  (b) seq_dev      Stereo.add_frames with the same device frames;
  (c) seq_host     Stereo.add_frames with host frames (uploads beside the matching).
Each figure is the median of --reps timed runs after --warmup untimed ones, with the spread
(min, max, and the inter-quartile range); the clock stops when the cloud's size is known on the
host, i.e. after the final synchronisation of each way.  One process, nothing else on the GPU.
Usage: python tools/stereo_sequence_probe.py [--reps 20] [--warmup 3] [--frames 9]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def stats(ms):
    import numpy as np
    a = np.sort(np.asarray(ms))
    q1, med, q3 = np.percentile(a, [25, 50, 75])
    return {"median_ms": round(float(med), 3), "min_ms": round(float(a[0]), 3),
            "max_ms": round(float(a[-1]), 3), "iqr_ms": round(float(q3 - q1), 3), "n": int(a.size)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=9)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    args = ap.parse_args()
    import torch
    import aerial_mapper_amd as A
    from aerial_mapper_amd import hip_lib
    import stereo_sequence as SS
    F, W, H = args.frames, args.width, args.height
    seq = SS.Sequence(F, W, H)
    Rs, ts = seq.camera_poses()
    dev = torch.from_numpy(seq.frames).cuda()
    host = [f for f in seq.frames]
    K = seq.K
    ncam = A.NCamera(K[0, 0], K[1, 1], K[0, 2], K[1, 2], W, H, T_C_B=seq.T_C_B)
    out = {"probe": "stereo_sequence", "frames": F, "width": W, "height": H,
           "build_id": hip_lib.build_id(), "device": torch.cuda.get_device_name(0)}
    with A.AerialGridMap(A.GridMapSettings(0.0, 0.0, 32.0, 32.0, 1.0)) as m:
        for name, use_bm in (("bm", True), ("sgbm", False)):
            bmp = A.BlockMatchingParameters(use_BM=use_bm)

            def pair_loop():
                n = 0
                for k in range(F - 1):
                    x, _ = A.dense_cloud_from_stereo_pair(m, K, Rs[k], Rs[k + 1], ts[k], ts[k + 1],
                                                          dev[k], dev[k + 1], bmp)
                    n += x.shape[0]
                return n

            with A.Stereo(ncam, A.StereoSettings(), bmp, m) as st:
                def seq_dev():
                    st.reset()
                    return st.add_frames(seq.T_G_B, dev)[0].shape[0]

                def seq_host():
                    st.reset()
                    return st.add_frames(seq.T_G_B, host)[0].shape[0]

                res = {}
                counts = set()
                # the three ways take turns inside every repetition, so that drift hits them alike
                ways = (("pair_loop", pair_loop), ("seq_dev", seq_dev), ("seq_host", seq_host))
                times = {k: [] for k, _ in ways}
                for rep in range(args.warmup + args.reps):
                    for key, fn in ways:
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        n = fn()
                        dt = (time.perf_counter() - t0) * 1e3
                        counts.add(n)
                        if rep >= args.warmup:
                            times[key].append(dt)
                for key, _ in ways:
                    res[key] = stats(times[key])
                assert len(counts) == 1, counts     # the three ways give the same cloud size
                res["points"] = counts.pop()
                res["seq_dev_minus_pair_loop_ms"] = round(res["seq_dev"]["median_ms"] -
                                                          res["pair_loop"]["median_ms"], 3)
                out[name] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
