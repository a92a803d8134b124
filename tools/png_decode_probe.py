"""One JSON line: what loading a PNG dataset's frames costs on one MI355X when the files are decoded
on the GPU (io.decode_png_frames / amhip_io_decode_png_frames).  249 frames of 1920 x 1080, gray and
RGB, written by Pillow at its default compression (--distinct N of them are made and repeated to 249;
every file is decoded as its own frame), of two contents: `synth`, synth's high-frequency frames,
where nearly every symbol of the stream is a literal, and `smooth`, slow ramps, where matches
dominate.  3 warm-up and --reps timed repeats, median and interquartile range, plus the library's
build id.
Columns: decode (bytes in host memory -> frames in HBM: parse, IDAT payloads joined, upload, three
kernels, status read-back), decode_to_host (the same plus DeviceFrames.to_host()), pillow
(Image.open(...).load() of the same files on one core: 1 warm-up and 3 repeats, recorded in its entry;
beside them, not a ratio to beat).
The result also goes to profiles/png_decode_probe_<build id>.json (--out FILE: elsewhere).
The split between the three kernels comes from a kernel trace of a fresh process:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python tools/png_decode_probe.py --trace-target
(its *_kernel_stats.csv lists the k_pngd_* kernels; DESIGN 4.12 quotes it).
Usage: python tools/png_decode_probe.py [--reps N] [--frames N] [--distinct N] [--out FILE] [--no-pillow] [--trace-target]"""
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


def smooth_frames(n, height, width, ch):
    import numpy as np
    y, x = np.mgrid[0:height, 0:width]
    out = []
    for k in range(n):
        g = ((x // 4 + y // 2 + 11 * k) & 255).astype(np.uint8)
        out.append(g if ch == 1 else np.stack([g, (g + 40) & 255, 255 - g], axis=2).astype(np.uint8))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=249)
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-pillow", action="store_true", help="do not time Pillow beside the GPU")
    ap.add_argument("--trace-target", action="store_true",
                    help="only decode every stack twice (the program to run under a kernel trace)")
    args = ap.parse_args()
    import numpy as np
    from PIL import Image      # (the files are Pillow's: the probe needs it)
    from aerial_mapper_amd import hip_lib, io as AIO, synth
    out = {"build_id": hip_lib.build_id(), "reps": args.reps, "warmup": 3, "frames": args.frames,
           "distinct_frames": args.distinct, "width": args.width, "height": args.height,
           "pillow": "left out" if args.no_pillow else "measured"}
    stacks = {}
    for content in ("synth", "smooth"):
        for name, ch in (("gray", 1), ("rgb", 3)):
            if content == "synth":
                frames = synth.make_frames(args.distinct, args.height, args.width, ch, salt=5)
            else:
                frames = smooth_frames(args.distinct, args.height, args.width, ch)
            files = []
            for f in frames:
                buf = io.BytesIO()
                Image.fromarray(np.ascontiguousarray(f)).save(buf, "PNG")
                files.append(buf.getvalue())
            stacks["%s_%s" % (content, name)] = [files[k % len(files)] for k in range(args.frames)]
    for name, files in stacks.items():
        colored = name.endswith("rgb")

        def decode():
            fr = AIO.decode_png_frames(files, colored=colored)
            fr.close()

        def decode_to_host():
            fr = AIO.decode_png_frames(files, colored=colored)
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
        if not args.no_pillow:
            def pillow():
                for f in files:
                    Image.open(io.BytesIO(f)).load()
            r["pillow"] = timed(pillow, PILLOW_REPS, warm=PILLOW_WARMUP)
            r["pillow"].update(reps=PILLOW_REPS, warmup=PILLOW_WARMUP)
        out[name] = r
    if args.trace_target:
        print(json.dumps({"trace_target": True, "build_id": hip_lib.build_id()}))
        return
    out["note"] = ("wall ms of synchronous calls from bytes in host memory; inflate uses one wave per frame "
                   "(sequential, wave-uniform), so its time is that of the longest stream of a group")
    line = json.dumps(out)
    print(line)
    path = args.out or os.path.join(ROOT, "profiles", "png_decode_probe_%s.json" % hip_lib.build_id())
    with open(path, "w") as fh_:
        fh_.write(line + "\n")


if __name__ == "__main__":
    main()
