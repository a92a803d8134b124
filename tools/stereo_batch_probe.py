"""One JSON line: what keeping n stereo pairs in flight buys.  F = 9 frames of 1920x1080 from
tests/stereo_sequence.py's generator, device frames, per matcher (BM, SGBM):
  parent      Stereo.add_frames of ANOTHER checkout of this project (--parent-tree: a tree with its own
              built library, e.g. the parent commit), measured by a second process that takes its turn
              inside every repetition of this one -- the same box, the same minutes; `parent_n8` is
              that tree with 8 pairs in flight;
  n1 .. n8    Stereo.add_frames of this tree with 1, 2, 4 and 8 pairs in flight.
The ways take turns inside every repetition (--warmup untimed, --reps timed), each figure is the
median with min, max and the inter-quartile range; the clock stops when the cloud's size is known on
the host.  Also: the matcher alone, one batched call of four 1920x1080 pairs against four one-pair
calls, by HIP events (`matcher_batch4`).
Usage: python tools/stereo_batch_probe.py [--parent-tree DIR] [--reps 20] [--warmup 3]
(--serve is the second process's mode: it answers one line per request "<matcher> <n>" on stdin.)"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stats(ms):
    import numpy as np
    a = np.sort(np.asarray(ms))
    q1, med, q3 = np.percentile(a, [25, 50, 75])
    return {"median_ms": round(float(med), 3), "min_ms": round(float(a[0]), 3),
            "max_ms": round(float(a[-1]), 3), "iqr_ms": round(float(q3 - q1), 3), "n": int(a.size)}


def setup(tree, args):
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(HERE, "tests"))   # (the generator: the same frames for both trees)
    import torch
    import aerial_mapper_amd as A
    import stereo_sequence as SS
    seq = SS.Sequence(args.frames, args.width, args.height)
    K = seq.K
    ncam = A.NCamera(K[0, 0], K[1, 1], K[0, 2], K[1, 2], args.width, args.height, T_C_B=seq.T_C_B)
    return torch, A, seq, ncam, torch.from_numpy(seq.frames).cuda()


def timed(torch, st, seq, dev):
    st.reset()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = st.add_frames(seq.T_G_B, dev)[0].shape[0]
    return (time.perf_counter() - t0) * 1e3, n


PARENT_WAYS = {"parent": 1, "parent_n8": 8}   # way -> pairs in flight of the other tree


def serve(args):
    torch, A, seq, ncam, dev = setup(args.serve, args)
    from aerial_mapper_amd import hip_lib
    with A.AerialGridMap(A.GridMapSettings(0.0, 0.0, 32.0, 32.0, 1.0)) as m:
        objs = {"%s %d" % (name, n): A.Stereo(ncam, A.StereoSettings(), A.BlockMatchingParameters(use_BM=bm), m,
                                              pairs_in_flight=n)
                for name, bm in (("bm", True), ("sgbm", False)) for n in PARENT_WAYS.values()}
        print(json.dumps({"ready": hip_lib.build_id()}), flush=True)
        for line in sys.stdin:
            name = line.strip()
            if name not in objs:
                break
            ms, n = timed(torch, objs[name], seq, dev)
            print(json.dumps({"ms": ms, "points": n}), flush=True)
        for st in objs.values():
            st.close()


def matcher_alone(torch, A, m, seq, use_bm, reps):
    """four rectified pairs: one batched call against four one-pair calls, HIP events"""
    Rs, ts = seq.camera_poses()
    K = seq.K
    dev = torch.from_numpy(seq.frames[:5]).cuda()
    rect = [A.rectify_stereo_pair(m, K, Rs[k], Rs[k + 1], ts[k], ts[k + 1], dev[k], dev[k + 1]) for k in range(4)]
    left = torch.stack([r["image_left"] for r in rect])
    right = torch.stack([r["image_right"] for r in rect])
    mask = torch.stack([r["mask"] for r in rect])
    fn = A.compute_disparity_bm if use_bm else A.compute_disparity_sgbm
    m.enable_timing(True)
    out = {}
    for key, call in (("four_calls", lambda: [fn(m, left[k], right[k], mask=mask[k]) for k in range(4)]),
                      ("one_batch", lambda: fn(m, left, right, mask=mask))):
        ms = []
        for rep in range(2 + reps):
            m.timing_reset()
            call()
            if rep >= 2:
                ms.append(m.kernel_times()["k_stereo"][0])
        out[key] = stats(ms)
    m.enable_timing(False)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=9)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--serve", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.serve:
        return serve(args)
    child = None
    out = {"probe": "stereo_batch", "frames": args.frames, "width": args.width, "height": args.height}
    if args.parent_tree:
        # a fresh child process (never a replaced one), with the other tree's package and library
        env = dict(os.environ)
        env.pop("AMHIP_LIB_PATH", None)
        child = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--serve", os.path.abspath(args.parent_tree),
                                  "--frames", str(args.frames), "--width", str(args.width),
                                  "--height", str(args.height)], stdin=subprocess.PIPE,
                                 stdout=subprocess.PIPE, universal_newlines=True, env=env)
        out["parent_build_id"] = json.loads(child.stdout.readline())["ready"]
    torch, A, seq, ncam, dev = setup(HERE, args)
    from aerial_mapper_amd import hip_lib
    out["build_id"] = hip_lib.build_id()
    out["device"] = torch.cuda.get_device_name(0)
    try:
        with A.AerialGridMap(A.GridMapSettings(0.0, 0.0, 32.0, 32.0, 1.0)) as m:
            for name, use_bm in (("bm", True), ("sgbm", False)):
                bmp = A.BlockMatchingParameters(use_BM=use_bm)
                objs = {n: A.Stereo(ncam, A.StereoSettings(), bmp, m, pairs_in_flight=n) for n in (1, 2, 4, 8)}
                ways = (list(PARENT_WAYS) if child else []) + ["n%d" % n for n in objs]
                times = {k: [] for k in ways}
                counts = set()
                for rep in range(args.warmup + args.reps):
                    for key in ways:       # (the ways take turns, so that drift hits them alike)
                        if key in PARENT_WAYS:
                            child.stdin.write("%s %d\n" % (name, PARENT_WAYS[key]))
                            child.stdin.flush()
                            r = json.loads(child.stdout.readline())
                            ms, n = r["ms"], r["points"]
                        else:
                            ms, n = timed(torch, objs[int(key[1:])], seq, dev)
                        counts.add(n)
                        if rep >= args.warmup:
                            times[key].append(ms)
                assert len(counts) == 1, counts      # every way gives the same cloud size
                res = {k: stats(v) for k, v in times.items()}
                res["points"] = counts.pop()
                for st in objs.values():
                    st.close()
                res["matcher_batch4"] = matcher_alone(torch, A, m, seq, use_bm, 10)
                out[name] = res
    finally:
        if child:
            child.stdin.write("quit\n")
            child.stdin.flush()
            child.wait(timeout=60)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
