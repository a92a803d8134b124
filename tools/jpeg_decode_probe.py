"""One JSON line: what loading the demo flags' frames costs on one MI355X when their JPEG files are
decoded on the GPU (io.decode_jpeg_frames / amhip_io_decode_jpeg_frames).  249 frames of 1920 x 1080,
gray and colour 4:2:0: synth's frames, encoded at quality 95 by the GPU encoder (--distinct N of them
are made and repeated to 249; every file is decoded as its own frame).  3 warm-up and 20 timed
repeats, median and interquartile range, plus the library's build id.
Columns: decode (bytes in host memory -> frames in HBM: parse, upload, three kernels, status
read-back), decode_to_host (the same plus DeviceFrames.to_host()), pillow (Image.open(...).load() of
the same files on one core, where Pillow is installed: 1 warm-up and 3 repeats, recorded in its
entry; beside them, not a ratio to beat).
The result also goes to profiles/jpeg_decode_probe_<build id>.json (--out FILE: elsewhere).
The split between the three kernels comes from a kernel trace of a fresh process:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python tools/jpeg_decode_probe.py --trace-target
(its *_kernel_stats.csv lists the k_jpegd_* kernels; DESIGN 4.11 quotes it).
--no-pillow leaves column (c) out: for timing two builds of the library in turn (AMHIP_LIB_PATH names
the other one), where Pillow's seconds per run buy nothing.
The progressive case (gray_progressive, colour_420_progressive) stands beside the baseline figures of
the same run: the same frames and pixels, written progressive (SOF2, libjpeg-turbo's default script)
by Pillow at quality 95 where Pillow is present, recorded in "progressive_writer".  Without Pillow:
--distinct-progressive N frames (default 1) through the symbol-level ProgressiveWriter of
tests/jpeg_progressive_inputs.py over tests/jpeg_reference.py's quantised coefficients, in Pillow's
script; the count is recorded.  --no-progressive leaves the case out (a library from before it
refuses SOF2).
Usage: python tools/jpeg_decode_probe.py [--reps N] [--frames N] [--distinct N] [--out FILE] [--no-pillow]
       [--no-progressive] [--distinct-progressive N] [--trace-target]"""
import argparse
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


# Pillow decodes 249 frames in seconds per repeat: fewer repeats, recorded beside its figures
PILLOW_REPS, PILLOW_WARMUP = 3, 1


def timed(fn, reps, warm=3):
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


def progressive_files(frames, ch, use_pillow):
    """the frames' pixels as progressive files at quality 95 (colour: 4:2:0) -> ([bytes], how)"""
    import numpy as np
    if use_pillow:
        from PIL import Image
        out = []
        for f in frames:
            pil = Image.fromarray(f if ch == 1 else np.ascontiguousarray(f[..., ::-1]))
            buf = io.BytesIO()
            pil.save(buf, "JPEG", quality=95, progressive=True, **({} if ch == 1 else {"subsampling": 2}))
            out.append(buf.getvalue())
        return out, "Pillow"
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import jpeg_progressive_inputs as PI
    import jpeg_reference as R
    out = []
    zz = [int(v) for v in R.ZIGZAG]
    for f in frames:
        b = R.blocks_of(f, 95)          # (zigzag order, in the order a baseline scan codes them)
        nat = np.zeros_like(b.coef)
        nat[:, zz] = b.coef
        h, wd = f.shape[:2]
        if ch == 1:
            comps, planes = [(1, 1, 1, 0)], [nat.reshape((h + 7) // 8, (wd + 7) // 8, 64)]
        else:
            my, mx = (h + 15) // 16, (wd + 15) // 16
            m = nat.reshape(my, mx, 6, 64)
            y = m[:, :, :4].reshape(my, mx, 2, 2, 64).transpose(0, 2, 1, 3, 4).reshape(2 * my, 2 * mx, 64)
            comps, planes = [(1, 2, 2, 0), (2, 1, 1, 1), (3, 1, 1, 1)], [y, m[:, :, 4], m[:, :, 5]]
        q = R.quant_tables(95)
        w = PI.ProgressiveWriter(wd, h, comps, {k: q[k] for k in range(1 if ch == 1 else 2)}, planes)
        n = len(comps)
        # libjpeg-turbo's default script (jpeg_simple_progression)
        sc = PI.scan
        if n == 1:
            script = [sc([0], 0, 0, 0, 1), sc([0], 1, 5, 0, 2), sc([0], 6, 63, 0, 2), sc([0], 1, 63, 2, 1),
                      sc([0], 0, 0, 1, 0), sc([0], 1, 63, 1, 0)]
        else:
            script = [sc([0, 1, 2], 0, 0, 0, 1, td=[0, 1, 1]), sc([0], 1, 5, 0, 2), sc([2], 1, 63, 0, 1, ta=1),
                      sc([1], 1, 63, 0, 1, ta=1), sc([0], 6, 63, 0, 2), sc([0], 1, 63, 2, 1), sc([0, 1, 2], 0, 0, 1, 0),
                      sc([2], 1, 63, 1, 0, ta=1), sc([1], 1, 63, 1, 0, ta=1), sc([0], 1, 63, 1, 0)]
        out.append(w.write(script))
    return out, "ProgressiveWriter"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=249)
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-pillow", action="store_true", help="do not time Pillow beside the GPU")
    ap.add_argument("--no-progressive", action="store_true", help="leave the progressive case out")
    ap.add_argument("--distinct-progressive", type=int, default=1,
                    help="distinct progressive frames where Pillow is not there to write them")
    ap.add_argument("--trace-target", action="store_true",
                    help="only decode both stacks twice (the program to run under a kernel trace)")
    args = ap.parse_args()
    import numpy as np
    import aerial_mapper_amd as A
    from aerial_mapper_amd import export as E, hip_lib, io as AIO, synth
    try:
        from PIL import Image
    except ImportError:
        Image = None
    have_pillow = Image is not None
    if args.no_pillow:
        Image = None
    out = {"build_id": hip_lib.build_id(), "reps": args.reps, "warmup": 3, "frames": args.frames,
           "distinct_frames": args.distinct, "width": args.width, "height": args.height,
           "pillow": "measured" if Image else "left out" if args.no_pillow else "not available"}
    stacks = {}
    with A.AerialGridMap(A.GridMapSettings(0.0, 0.0, 32.0, 32.0, 1.0), device=0) as m:
        for name, ch in (("gray", 1), ("colour_420", 3)):
            frames = synth.make_frames(args.distinct, args.height, args.width, ch, salt=5)
            files = [E.encode_jpeg(m, np.ascontiguousarray(f), 95) for f in frames]
            stacks[name] = [files[k % len(files)] for k in range(args.frames)]
            if not args.no_progressive:
                some = frames if have_pillow else frames[:max(1, args.distinct_progressive)]
                files, how = progressive_files([np.ascontiguousarray(f) for f in some], ch, have_pillow)
                stacks[name + "_progressive"] = [files[k % len(files)] for k in range(args.frames)]
                out["progressive_writer"] = how
                out["distinct_progressive_frames"] = len(files)
    for name, files in stacks.items():
        colored = not name.startswith("gray")

        def decode():
            fr = AIO.decode_jpeg_frames(files, colored=colored)
            fr.close()

        def decode_to_host():
            fr = AIO.decode_jpeg_frames(files, colored=colored)
            fr.to_host()
            fr.close()

        if args.trace_target:
            decode()
            decode()
            continue
        r = {"file_bytes_total": int(sum(len(f) for f in files)),
             "file_bytes_mean": float(np.mean([len(f) for f in files])),
             "pixels_total": args.frames * args.width * args.height}
        r["decode"] = timed(decode, args.reps)
        r["decode_to_host"] = timed(decode_to_host, args.reps)
        if Image:
            def pillow():
                for f in files:
                    im = Image.open(io.BytesIO(f))
                    if not colored:
                        im.draft("L", im.size)
                    im.load()
            r["pillow"] = timed(pillow, PILLOW_REPS, warm=PILLOW_WARMUP)
            r["pillow"].update(reps=PILLOW_REPS, warmup=PILLOW_WARMUP)
        out[name] = r
    if args.trace_target:
        print(json.dumps({"trace_target": True, "build_id": hip_lib.build_id()}))
        return
    out["note"] = ("wall ms of synchronous calls from bytes in host memory; the entropy walk uses one wave per frame "
                   "(sequential, on the scalar unit), so its time is that of the longest scan of a group")
    line = json.dumps(out)
    print(line)
    path = args.out or os.path.join(ROOT, "profiles", "jpeg_decode_probe_%s.json" % hip_lib.build_id())
    with open(path, "w") as fh_:
        fh_.write(line + "\n")


if __name__ == "__main__":
    main()
