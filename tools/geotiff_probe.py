"""One JSON line: what writing a map layer as tiled Deflate GeoTIFF costs on one MI355X when it is
compressed on the GPU (export.layer_to_geotiff, amhip_tiff_encode.hip), beside what existed before
for the same layer: the raw download plus amhip_geotiff_write_u8 of its 8-bit image, and layer_to_png.
Inputs, on a --side x --side map at 0.25 m (default 10 000, bench.py's cfg3 map):
  elevation_f32   the `elevation` the bench's DSM leaves (--points synth points, radius_sq 1), as f32
  ortho_u8        an `ortho` layer of smooth terrain shading with empty cells, as u8 (0..255)
  colour_rgb8     a packed colour layer covered to 38 % with synth's high-frequency pixels, as rgb8
  all_nan_f32     the map as initialised
Columns: raw_bytes (the raster), file_bytes, encode (layer in HBM -> file in HBM, size read back), write
(the same plus download and the file on disk), download_plus_u8 (amhip_layer_download of the layer plus
layer_to_image and amhip_geotiff_write_u8: the uncompressed 8-bit way out), png (layer_to_png); the two 8-bit
ways rescale `elevation` from 380..420 m.  3 warm-up
and --reps timed repeats in one process, median and interquartile range; wall ms of synchronous calls.
Every file is read back through tests/geotiff_reference.py's inverse once and compared with the layer.
The result also goes to profiles/geotiff_probe_<build id>.json (--out FILE: elsewhere).
The split between the kernels comes from a kernel trace of a fresh process:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python tools/geotiff_probe.py --trace-target
Usage: python tools/geotiff_probe.py [--reps N] [--side N] [--points N] [--tile N] [--out FILE] [--trace-target]"""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--side", type=int, default=10000)
    ap.add_argument("--points", type=int, default=50_000_000)
    ap.add_argument("--tile", type=int, default=256)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-target", action="store_true",
                    help="only encode every input twice (the program to run under a kernel trace)")
    args = ap.parse_args()
    import numpy as np
    import torch
    import aerial_mapper_amd as A
    from aerial_mapper_amd import export as E, hip_lib, synth
    import geotiff_reference as GR
    lib = hip_lib.load()
    n, res = args.side, 0.25
    out = {"build_id": hip_lib.build_id(), "reps": args.reps, "warmup": 3, "side": n, "tile": args.tile,
           "points": args.points}
    tmp = tempfile.mkdtemp(prefix="geotiff_probe_")
    try:
        with A.AerialGridMap(A.GridMapSettings(0.0, 0.0, n * res, n * res, res), device=0) as m:
            dev = torch.device("cuda:0")
            bound = lib.amhip_geotiff_bound(n, n, 0, args.tile)   # (f32: the largest of the three kinds)
            buf = torch.empty(int(bound), dtype=torch.uint8, device=dev)
            host = np.empty((n, n), np.float32)
            size = C.c_size_t()

            def encode(layer, kind, lo, hi):
                hip_lib.check(lib.amhip_layer_encode_geotiff_dev(
                    m._h, hip_lib.LAYER_NAMES.index(layer), hip_lib.GEOTIFF_KINDS[kind], lo, hi, args.tile, 32, 1,
                    C.c_void_p(buf.data_ptr()), int(bound), C.byref(size)))
                return size.value

            def measure(name, layer, kind, lo, hi):
                if args.trace_target:
                    encode(layer, kind, lo, hi)
                    encode(layer, kind, lo, hi)
                    return
                px = {"f32": 4, "u8": 1, "rgb8": 3}[kind]
                f = os.path.join(tmp, name + ".tif")
                r = {"raw_bytes": n * n * px, "file_bytes": int(encode(layer, kind, lo, hi))}
                r["encode"] = timed(lambda: encode(layer, kind, lo, hi), args.reps)
                r["write"] = timed(lambda: E.layer_to_geotiff(m, layer, f, kind, lo, hi, 32, True, args.tile), args.reps)
                assert os.path.getsize(f) == r["file_bytes"]
                back = GR.decode(open(f, "rb").read())
                want = GR.layer_raster(m.get(layer), kind, lo, hi)
                assert np.array_equal(back["raster"].view(np.uint8), want.view(np.uint8)), name
                bgr = kind == "rgb8"
                gt = (C.c_double * 6)(*back["geotransform"])

                def old_way():
                    m.get(layer, out=host)
                    img = E.layer_to_image(m, layer, lo, hi, bgr=bgr)
                    E.write_geotiff(f + ".u8.tif", img, gt)

                r["download_plus_u8"] = timed(old_way, max(3, args.reps // 4), warm=1)
                r["png"] = timed(lambda: E.layer_to_png(m, layer, f + ".png", lo, hi, bgr=bgr), max(3, args.reps // 4),
                                 warm=1)
                r["png_bytes"] = os.path.getsize(f + ".png")
                out[name] = r
                for p in (f, f + ".u8.tif", f + ".png"):
                    os.remove(p)

            measure("all_nan_f32", "elevation", "f32", 0.0, 255.0)
            pts = synth.make_points_torch(args.points, n * res / 2.0, 43, dev)
            A.Dsm(A.DsmSettings(1), m).process(pts, m)
            del pts
            measure("elevation_f32", "elevation", "f32", 380.0, 420.0)   # (the range of the two 8-bit ways)
            y, x = np.mgrid[0:n, 0:n]
            rng = np.random.default_rng(3)
            ortho = ((np.sin(x / 97.0) + np.cos(y / 131.0)) * 60 + 128 + rng.integers(0, 6, (n, n))).astype(np.float32)
            ortho[(x + 2 * y) % 4096 < 300] = np.nan                  # cells nothing was observed in
            del x, y
            m.set("ortho", ortho)
            del ortho
            measure("ortho_u8", "ortho", "u8", 0.0, 255.0)
            packed = np.full((n, n), np.nan, np.float32)
            covered = int(n * 0.38)
            px = synth.make_frames(1, n, covered, 3, salt=7)[0].astype(np.uint32)
            packed.view(np.uint32)[:, :covered] = (px[:, :, 0] << 16) | (px[:, :, 1] << 8) | px[:, :, 2]
            del px
            m.set("colored_ortho", packed)
            del packed
            measure("colour_rgb8", "colored_ortho", "rgb8", 0.0, 255.0)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    if args.trace_target:
        print(json.dumps({"trace_target": True, "build_id": hip_lib.build_id()}))
        return
    out["note"] = ("wall ms of synchronous calls on layers in HBM; write / download_plus_u8 / png: to a temporary "
                   "directory of the local disk; download_plus_u8 and png are the ways out that existed before")
    line = json.dumps(out)
    print(line)
    path = args.out or os.path.join(ROOT, "profiles", "geotiff_probe_%s.json" % hip_lib.build_id())
    with open(path, "w") as fh_:
        fh_.write(line + "\n")


if __name__ == "__main__":
    main()
