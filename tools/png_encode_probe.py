"""One JSON line: what writing PNG files costs on one MI355X when they are encoded on the GPU
(io.encode_png_frames / write_png_frames, amhip_png_encode.hip), beside the JPEG path on the same
input and two host encoders on one core.
Inputs: 249 frames of 1920 x 1080, gray and colour (--distinct N of them are made and repeated to
249; every frame is encoded as its own file), of two contents: `synth`, synth's high-frequency
frames, where nearly every symbol is a literal, and `smooth`, slow ramps of steps four pixels wide,
where runs dominate; a 10 000 x 10 000 gray raster (cfg3's `ortho` layer: smooth terrain shading with
empty cells); a 10 000 x 10 000 colour mosaic covered to 38 %.
Columns: encode (frames in HBM -> files in HBM, sizes read back), write (the same plus download and the
files on disk), jpeg_encode / jpeg_write (quality 95, the same input), pillow
(Image.save(compress_level=1)) and zlib_rle (compressobj(1, DEFLATED, 15, 8, Z_RLE) on the Sub-filtered
scanlines, filter not timed), each on one core over --host-frames frames and scaled to the stack's frame
count in `scaled_ms`.  3 warm-up and --reps timed repeats, median and interquartile range.  No ratio is
claimed.  `file_bytes` is what the device wrote, `zlib_rle_stream_bytes` what zlib's Z_RLE stream plus
the container comes to for the same frames: the two must be equal, and the probe fails when they are not.
The result also goes to profiles/png_encode_probe_<build id>.json (--out FILE: elsewhere).
The split between the kernels comes from a kernel trace of a fresh process:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python tools/png_encode_probe.py --trace-target
(its *_kernel_stats.csv lists the k_pnge_* kernels; DESIGN 4.15 quotes it).
Usage: python tools/png_encode_probe.py [--reps N] [--frames N] [--distinct N] [--side N] [--out FILE] [--trace-target]"""
import argparse
import io
import json
import os
import shutil
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HOST_REPS, HOST_WARMUP = 3, 1


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


def scanlines(px):
    import numpy as np
    p = px[:, :, None] if px.ndim == 2 else px[:, :, ::-1]
    h, w, c = p.shape
    row = p.reshape(h, w * c).astype(np.int16)
    sub = row.copy()
    sub[:, c:] -= row[:, :-c]
    out = np.empty((h, 1 + w * c), np.uint8)
    out[:, 0] = 1
    out[:, 1:] = sub.astype(np.uint8)
    return out.tobytes()


def rle_stream(raw):
    c = zlib.compressobj(1, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
    return c.compress(raw) + c.flush()


def file_size(z):
    return 33 + z + 12 * -(-z // 8192) + 12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=249)
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--side", type=int, default=10000, help="side of the layer and of the mosaic")
    ap.add_argument("--host-frames", type=int, default=4)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-target", action="store_true",
                    help="only encode every input twice (the program to run under a kernel trace)")
    args = ap.parse_args()
    import numpy as np
    import torch
    from PIL import Image
    from aerial_mapper_amd import hip_lib, io as AIO, synth
    out = {"build_id": hip_lib.build_id(), "reps": args.reps, "warmup": 3, "frames": args.frames,
           "distinct_frames": args.distinct, "width": args.width, "height": args.height, "side": args.side,
           "host_reps": HOST_REPS, "host_warmup": HOST_WARMUP, "host_frames": args.host_frames}
    inputs = {}
    for content in ("synth", "smooth"):
        for name, ch in (("gray", 1), ("rgb", 3)):
            if content == "synth":
                frames = synth.make_frames(args.distinct, args.height, args.width, ch, salt=5)
            else:
                frames = smooth_frames(args.distinct, args.height, args.width, ch)
            frames = [np.ascontiguousarray(f) for f in frames]
            inputs["%s_%s" % (content, name)] = [frames[k % len(frames)] for k in range(args.frames)]
    n = args.side
    rng = np.random.default_rng(3)
    y, x = np.mgrid[0:n, 0:n]
    layer = ((np.sin(x / 97.0) + np.cos(y / 131.0)) * 60 + 128 + rng.integers(0, 6, (n, n))).astype(np.uint8)
    layer[(x + 2 * y) % 4096 < 300] = 0                     # cells nothing was observed in
    inputs["ortho_layer_gray"] = [layer]
    mosaic = np.zeros((n, n, 3), np.uint8)
    covered = int(n * 0.38)
    mosaic[:, :covered] = synth.make_frames(1, n, covered, 3, salt=7)[0]
    inputs["mosaic_38pct_rgb"] = [mosaic]
    del x, y
    tmp = tempfile.mkdtemp(prefix="png_encode_probe_")
    try:
        for name, frames in inputs.items():
            distinct = frames[:args.distinct]
            dev = torch.from_numpy(np.stack(distinct)).cuda()
            index = torch.arange(len(frames), device="cuda") % len(distinct)
            stack = dev[index].contiguous() if len(frames) > len(distinct) else dev
            torch.cuda.synchronize()
            names_png = [os.path.join(tmp, "%s_%d.png" % (name, k)) for k in range(len(frames))]
            names_jpg = [os.path.join(tmp, "%s_%d.jpg" % (name, k)) for k in range(len(frames))]
            if args.trace_target:
                AIO.encode_png_frames(stack)
                AIO.encode_png_frames(stack)
                continue
            lib = hip_lib.load()
            import ctypes as C

            def encode(symbol, *quality):
                ptr, _, f, w, h, ch, row, stride, keep = AIO._frames_arg(stack, 0, True)
                res = C.c_void_p()
                offsets = (C.c_size_t * (f + 1))()
                hip_lib.check(getattr(lib, symbol)(0, C.c_void_p(ptr), f, w, h, ch, row, stride, *quality,
                                                   C.byref(res), offsets))
                lib.amhip_io_free(res)
                return offsets[f]

            r = {"pixels_total": int(len(frames) * frames[0].shape[0] * frames[0].shape[1]),
                 "file_bytes": int(encode("amhip_io_encode_png_frames")),
                 "jpeg_file_bytes": int(encode("amhip_io_encode_jpeg_frames", 95))}
            r["encode"] = timed(lambda: encode("amhip_io_encode_png_frames"), args.reps)
            r["write"] = timed(lambda: AIO.write_png_frames(stack, names_png), args.reps)
            r["jpeg_encode"] = timed(lambda: encode("amhip_io_encode_jpeg_frames", 95), args.reps)
            r["jpeg_write"] = timed(lambda: AIO.write_jpeg_frames(stack, names_jpg, 95), args.reps)
            assert sum(os.path.getsize(p) for p in names_png) == r["file_bytes"]
            host = distinct[:args.host_frames]
            scale = len(frames) / float(len(host))
            raws = [scanlines(f) for f in host]
            streams = [rle_stream(raw) for raw in raws]
            # the device's files against zlib's streams: the same bytes, so the same sizes
            got = AIO.encode_png_frames(np.stack(host))
            for g, z in zip(got, streams):
                assert len(g) == file_size(len(z)) and z in (b"".join(
                    g[at + 8:at + 8 + int.from_bytes(g[at:at + 4], "big")] for at in _idats(g)),), name
            per_frame = {}
            for k, f in enumerate(frames):
                per_frame.setdefault(k % len(distinct), 0)
                per_frame[k % len(distinct)] += 1
            if len(distinct) <= args.host_frames:
                r["zlib_rle_stream_bytes"] = int(sum(file_size(len(streams[k])) * c for k, c in per_frame.items()))
                assert r["zlib_rle_stream_bytes"] == r["file_bytes"], name
            else:
                r["zlib_rle_stream_bytes_of_host_frames"] = int(sum(file_size(len(z)) for z in streams))
                r["file_bytes_of_host_frames"] = int(sum(len(g) for g in got))
                assert r["zlib_rle_stream_bytes_of_host_frames"] == r["file_bytes_of_host_frames"], name

            def pillow():
                for f in host:
                    Image.fromarray(f if f.ndim == 2 else f[:, :, ::-1]).save(io.BytesIO(), "PNG", compress_level=1)

            def zlib_rle():
                for raw in raws:
                    rle_stream(raw)

            for key, fn in (("pillow", pillow), ("zlib_rle", zlib_rle)):
                r[key] = timed(fn, HOST_REPS, warm=HOST_WARMUP)
                r[key]["scaled_ms"] = r[key]["median_ms"] * scale
            out[name] = r
            del stack, dev
            for p in names_png + names_jpg:
                if os.path.exists(p):
                    os.remove(p)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    if args.trace_target:
        print(json.dumps({"trace_target": True, "build_id": hip_lib.build_id()}))
        return
    out["note"] = ("wall ms of synchronous calls on frames in HBM; write: to a temporary directory of the local disk; "
                   "host encoders: one core, host_frames frames, scaled_ms = median * frames / host_frames")
    line = json.dumps(out)
    print(line)
    path = args.out or os.path.join(ROOT, "profiles", "png_encode_probe_%s.json" % hip_lib.build_id())
    with open(path, "w") as fh_:
        fh_.write(line + "\n")


def _idats(g):
    at, out = 33, []
    while g[at + 4:at + 8] == b"IDAT":
        out.append(at)
        at += 12 + int.from_bytes(g[at:at + 4], "big")
    return out


if __name__ == "__main__":
    main()
