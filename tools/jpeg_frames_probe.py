"""One JSON line: what writing a stack of frames as JPEG files costs on one MI355X through the batched
encoder (amhip_io_encode_jpeg_frames / amhip_io_write_jpeg_frames), next to the loop over the
single-image calls (amhip_jpeg_encode_dev / amhip_jpeg_write) on the same frames, in one process.
Both routes write identical files (checked here once per stack), so the ratio compares like with like.
Stacks, resident in HBM: 64 x (752 x 480 gray), 249 x (1920 x 1080 gray), 64 x (1920 x 1080 colour);
synthetic texture (smooth shading plus mild noise, every frame different).
  encode: (a) amhip_io_encode_jpeg_frames  vs  (b) F x amhip_jpeg_encode_dev into one worst-case buffer
  write:  (c) amhip_io_write_jpeg_frames   vs      F x amhip_jpeg_write, to a temporary directory
Warm-up plus repeats, median and interquartile range of the wall ms of the synchronous calls, keyed by
the library's build id.  The result also goes to profiles/jpeg_frames_probe_<build id>.json (--out FILE:
elsewhere).  Where the time goes, kernel by kernel:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python tools/jpeg_frames_probe.py --trace-target
(a fresh process that only runs (a) and (b) on the 64 small frames five times each).
Usage: python tools/jpeg_frames_probe.py [--reps N] [--warmup N] [--out FILE] [--trace-target]"""
import argparse
import ctypes as C
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STACKS = [("64x752x480_gray", 64, 752, 480, 1), ("249x1920x1080_gray", 249, 1920, 1080, 1),
          ("64x1920x1080_colour", 64, 1920, 1080, 3)]


def timed(fn, reps, warm):
    import numpy as np
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    q1, med, q3 = np.percentile(ms, [25, 50, 75])
    return {"median_ms": float(med), "iqr_ms": float(q3 - q1)}


def make_stack(n, w, h, ch):
    """smooth shading that moves from frame to frame, plus noise of +-6: files of a camera's size"""
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(1000 * n + ch)
    y = torch.arange(h, device="cuda", dtype=torch.float32)[None, :, None]
    x = torch.arange(w, device="cuda", dtype=torch.float32)[None, None, :]
    f = torch.arange(n, device="cuda", dtype=torch.float32)[:, None, None]
    out = torch.empty((n, h, w) + ((3,) if ch == 3 else ()), dtype=torch.uint8, device="cuda")
    for c in range(ch):
        v = 128 + 60 * torch.sin(x / (37.0 + 5 * c) + 0.1 * f) * torch.cos(y / 53.0 - 0.07 * f) + 40 * torch.sin((x + 2 * y) / 11.0)
        v = v + torch.randint(-6, 7, v.shape, device="cuda", generator=g)
        if ch == 3:
            out[..., c] = v.clamp(0, 255).to(torch.uint8)
        else:
            out[...] = v.clamp(0, 255).to(torch.uint8)
    torch.cuda.synchronize()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-target", action="store_true",
                    help="only the two encode routes on the 64 small frames, five times each (for a kernel trace)")
    args = ap.parse_args()
    import torch
    import aerial_mapper_amd as A
    from aerial_mapper_amd import hip_lib, io as AIO
    lib = hip_lib.load()
    out = {"build_id": hip_lib.build_id(), "reps": args.reps, "warmup": args.warmup, "stacks": {}}
    tmp = tempfile.mkdtemp(prefix="jpeg_frames_probe")
    with A.AerialGridMap(A.GridMapSettings(0.0, 0.0, 8.0, 8.0, 1.0), device=0) as m:
        for name, n, w, h, ch in STACKS[:1] if args.trace_target else STACKS:
            stack = make_stack(n, w, h, ch)
            ptr, row, stride = stack.data_ptr(), stack.stride(1), stack.stride(0)
            bound = lib.amhip_jpeg_bound(w, h, ch)
            one = torch.empty(bound, dtype=torch.uint8, device="cuda")
            nbytes = C.c_size_t()
            offsets = (C.c_size_t * (n + 1))()

            def batch():
                dev = C.c_void_p()
                hip_lib.check(lib.amhip_io_encode_jpeg_frames(0, C.c_void_p(ptr), n, w, h, ch, row, stride, 95,
                                                              C.byref(dev), offsets))
                lib.amhip_io_free(dev)

            def loop():
                for f in range(n):
                    hip_lib.check(lib.amhip_jpeg_encode_dev(m._h, C.c_void_p(ptr + f * stride), row, w, h, ch, 95,
                                                            C.c_void_p(one.data_ptr()), bound, C.byref(nbytes)))
            if args.trace_target:
                for _ in range(5):
                    batch()
                    loop()
                print(json.dumps({"trace_target": True, "stack": name, "build_id": hip_lib.build_id()}))
                return
            r = {"frames": n, "width": w, "height": h, "channels": ch}
            r["encode_batch"] = timed(batch, args.reps, args.warmup)
            r["encode_loop"] = timed(loop, args.reps, args.warmup)
            r["file_bytes"] = int(offsets[n])
            a_dir, b_dir = os.path.join(tmp, name + "_batch"), os.path.join(tmp, name + "_loop")
            os.makedirs(a_dir)
            os.makedirs(b_dir)
            a_names = [os.path.join(a_dir, "image_%d.jpg" % f) for f in range(n)]
            b_names = [os.path.join(b_dir, "image_%d.jpg" % f).encode() for f in range(n)]

            def write_loop():
                for f in range(n):
                    hip_lib.check(lib.amhip_jpeg_write(m._h, b_names[f], C.c_void_p(ptr + f * stride), 1, row, w, h,
                                                       ch, 95))
            r["write_batch"] = timed(lambda: AIO.write_jpeg_frames(stack, a_names, 95), args.reps, args.warmup)
            r["write_loop"] = timed(write_loop, args.reps, args.warmup)
            same = all(open(a_names[f], "rb").read() == open(b_names[f].decode(), "rb").read() for f in range(n))
            r["files_identical"] = bool(same)
            r["encode_loop_over_batch"] = r["encode_loop"]["median_ms"] / r["encode_batch"]["median_ms"]
            r["write_loop_over_batch"] = r["write_loop"]["median_ms"] / r["write_batch"]["median_ms"]
            out["stacks"][name] = r
            shutil.rmtree(a_dir)
            shutil.rmtree(b_dir)
            del stack, one
    shutil.rmtree(tmp, ignore_errors=True)
    out["note"] = ("wall ms of synchronous calls on frames resident in HBM; encode_batch includes allocating and "
                   "freeing the result; encode_loop writes every file into one reused worst-case buffer")
    line = json.dumps(out)
    print(line)
    path = args.out or os.path.join(ROOT, "profiles", "jpeg_frames_probe_%s.json" % hip_lib.build_id())
    with open(path, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
