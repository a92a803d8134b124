"""One JSON line: what loading a DEM from a tiled Deflate GeoTIFF into the `elevation` layer costs on one
MI355X when it is decoded on the GPU (io.layer_from_geotiff, amhip_tiff_decode.hip), beside what a user
did before: libtiff through Pillow on the host (where Pillow is absent: zlib.decompress per tile plus
numpy) and amhip_layer_upload of the result.
Input: a --side x --side f32 terrain (default 10 000, bench.py's cfg3 map at 0.25 m) written by
export.write_geotiff_deflate at --tile (default 256) with the map's own geotransform, so that every
cell takes a pixel.
Columns (wall ms of synchronous calls; 2 warm-up and --reps timed repeats in one process, median and
interquartile range):
  layer_from_geotiff   file bytes in host memory -> layer in HBM: parse, pack, upload, inflate, unpredict, place
  decode_geotiff       the same without the placement, into a device raster that exists already
  host_then_upload     the way that existed before
The split of the device time between the kernels (k_pngd_inflate, k_tiffd_unpredict, k_tiffd_place) and
what is left for the host (parse, pack, upload) comes from a kernel trace of a fresh process:
  rocprofv3 --kernel-trace --stats -d DIR -o t -- python tools/geotiff_read_probe.py --trace-target
The result also goes to profiles/geotiff_read_probe_<build id>.json (--out FILE: elsewhere).
Usage: python tools/geotiff_read_probe.py [--reps N] [--side N] [--tile N] [--out FILE] [--trace-target]"""
import argparse
import ctypes as C
import io as _io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn, reps, warm=2):
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
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--side", type=int, default=10000)
    ap.add_argument("--tile", type=int, default=256)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-target", action="store_true",
                    help="only load the file twice (the program to run under a kernel trace)")
    args = ap.parse_args()
    import numpy as np
    import torch
    import aerial_mapper_amd as A
    from aerial_mapper_amd import hip_lib
    import geotiff_read_reference as R
    lib = hip_lib.load()
    n, res = args.side, 0.25
    out = {"build_id": hip_lib.build_id(), "reps": args.reps, "warmup": 2, "side": n, "tile": args.tile}
    with A.AerialGridMap(A.GridMapSettings(0.0, 0.0, n * res, n * res, res), device=0) as m:
        # SURVEY's 400 + 10 sin cos surface with a centimetre of noise: the low mantissa planes do not collapse
        y, x = np.mgrid[0:n, 0:n].astype(np.float32) * np.float32(res)
        rng = np.random.default_rng(5)
        terrain = (400.0 + 10.0 * np.sin(x / 7.0) * np.cos(y / 5.0)).astype(np.float32)
        terrain += (rng.random((n, n), dtype=np.float32) - np.float32(0.5)) * np.float32(0.01)
        del x, y
        gt = (-n * res / 2, res, 0.0, n * res / 2, 0.0, -res)
        data = A.encode_geotiff(m, terrain, gt, 32, True, args.tile)
        out["raw_bytes"], out["file_bytes"] = int(terrain.nbytes), len(data)
        lid = hip_lib.LAYER_NAMES.index("elevation")

        def load():
            hip_lib.check(lib.amhip_layer_decode_geotiff(m._h, lid, data, len(data)))

        if args.trace_target:
            load()
            load()
            print(json.dumps({"trace_target": True, "build_id": hip_lib.build_id()}))
            return
        raster = torch.empty((n, n), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()

        def decode():
            hip_lib.check(lib.amhip_geotiff_decode_dev(m._h, data, len(data), 0, 0, n, n, C.c_void_p(raster.data_ptr()),
                                                       4 * n))

        out["layer_from_geotiff"] = timed(load, args.reps)
        got = m.get("elevation")
        assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(terrain[:, ::-1]).view(np.uint32))
        del got
        out["decode_geotiff"] = timed(decode, args.reps)
        assert np.array_equal(raster.cpu().numpy().view(np.uint32), terrain.view(np.uint32))
        try:
            from PIL import Image
            Image.MAX_IMAGE_PIXELS = None
            out["host_decoder"] = "libtiff through Pillow"

            def host_raster():
                return np.asarray(Image.open(_io.BytesIO(data)))
            host_raster()
        except Exception:     # (no Pillow, or one whose libtiff does not take the file)
            out["host_decoder"] = "zlib.decompress per tile + numpy"

            def host_raster():
                return R.decode(data)[0]
        host_ms = {}

        def old_way():
            t0 = time.perf_counter()
            north = host_raster()
            t1 = time.perf_counter()
            m.set("elevation", np.ascontiguousarray(north[:, ::-1]))     # (the layer's orientation: x falls with i)
            host_ms.setdefault("decode", []).append((t1 - t0) * 1e3)
            host_ms.setdefault("flip_upload", []).append((time.perf_counter() - t1) * 1e3)

        out["host_then_upload"] = timed(old_way, max(3, args.reps // 2), warm=1)
        out["host_then_upload"]["decode_median_ms"] = float(np.median(host_ms["decode"][1:]))
        out["host_then_upload"]["flip_upload_median_ms"] = float(np.median(host_ms["flip_upload"][1:]))
        assert np.array_equal(m.get("elevation").view(np.uint32), np.ascontiguousarray(terrain[:, ::-1]).view(np.uint32))
    out["note"] = ("wall ms of synchronous calls; the file's bytes are in host memory in both ways; the kernels' "
                   "shares come from a kernel trace of --trace-target in a run of its own")
    line = json.dumps(out)
    print(line)
    path = args.out or os.path.join(ROOT, "profiles", "geotiff_read_probe_%s.json" % hip_lib.build_id())
    with open(path, "w") as fh_:
        fh_.write(line + "\n")


if __name__ == "__main__":
    main()
