"""One JSON line: what GeoTIFF overviews cost going out and save coming in on one MI355X.
Input: a --side x --side f32 terrain (default 10 000, bench.py's cfg3 map at 0.25 m: SURVEY's surface plus
a centimetre of noise, the input of tools/geotiff_read_probe.py) and a byte image of it, as device
rasters, at --tile (default 256).
Columns (wall ms of synchronous calls; 2 warm-up and --reps timed repeats in one process, median and
interquartile range):
  encode_ovr0 / encode_ovr_auto    amhip_geotiff_encode_ovr_dev with overviews 0 and -1, per kind (f32, u8): raster
                                   in HBM -> file in HBM, its size read back
  layer_level0 / layer_auto        layer_from_geotiff of the f32 pyramid onto a (side / 4)^2 map at 1 m over
                                   the same ground, level=0 against level=-1 (which takes level 2)
The reduction kernels' share of the encoder's kernel time comes from a kernel trace of a fresh process:
  rocprofv3 --kernel-trace --stats -d DIR -o t -- python tools/geotiff_pyramid_probe.py --trace-target
The result also goes to profiles/geotiff_pyramid_probe_<build id>.json (--out FILE: elsewhere).
Usage: python tools/geotiff_pyramid_probe.py [--reps N] [--side N] [--tile N] [--out FILE] [--trace-target]"""
import argparse
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
                    help="only encode the f32 pyramid twice (the program to run under a kernel trace)")
    args = ap.parse_args()
    import numpy as np
    import torch
    import aerial_mapper_amd as A
    from aerial_mapper_amd import hip_lib
    import geotiff_pyramid_reference as P
    n, res = args.side, 0.25
    out = {"build_id": hip_lib.build_id(), "reps": args.reps, "warmup": 2, "side": n, "tile": args.tile}
    y, x = np.mgrid[0:n, 0:n].astype(np.float32) * np.float32(res)
    rng = np.random.default_rng(5)
    terrain = (400.0 + 10.0 * np.sin(x / 7.0) * np.cos(y / 5.0)).astype(np.float32)
    terrain += (rng.random((n, n), dtype=np.float32) - np.float32(0.5)) * np.float32(0.01)
    del x, y
    gt = (-n * res / 2, res, 0.0, n * res / 2, 0.0, -res)
    with A.AerialGridMap(A.GridMapSettings(0.0, 0.0, 8.0, 8.0, 1.0), device=0) as m:
        dev = {"f32": torch.from_numpy(terrain).to("cuda:0")}
        dev["u8"] = ((dev["f32"] - 389.0) * (255.0 / 22.0)).clamp(0, 255).to(torch.uint8)
        torch.cuda.synchronize()
        if args.trace_target:
            for _ in range(2):
                A.encode_geotiff(m, dev["f32"], gt, 32, True, args.tile, overviews=-1)
            print(json.dumps({"trace_target": True, "build_id": hip_lib.build_id()}))
            return
        import ctypes as C
        lib = hip_lib.load()
        gtc = (C.c_double * 6)(*gt)
        nbytes = C.c_size_t()
        cap = int(lib.amhip_geotiff_bound_ovr(n, n, 0, args.tile, -1))
        buf = torch.empty(cap, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()

        def encode(kind, ovr):     # raster in HBM -> file in HBM, its size read back
            t = dev[kind]
            hip_lib.check(lib.amhip_geotiff_encode_ovr_dev(m._h, C.c_void_p(t.data_ptr()), t.stride(0) * t.element_size(),
                                                           n, n, hip_lib.GEOTIFF_KINDS[kind], args.tile, ovr, gtc, 32, 1,
                                                           C.c_void_p(buf.data_ptr()), cap, C.byref(nbytes)))

        for kind in ("f32", "u8"):
            for name, ovr in (("encode_ovr0", 0), ("encode_ovr_auto", -1)):
                out["%s_%s" % (name, kind)] = timed(lambda: encode(kind, ovr), args.reps)
                out["%s_%s" % (name, kind)]["file_bytes"] = int(nbytes.value)
        encode("f32", -1)
        data = buf[:nbytes.value].cpu().numpy().tobytes()
        del buf
        infos = A.geotiff_levels(data)
        out["levels"] = [(d["width"], d["height"]) for d in infos]
        # level 1 of the GPU's file against numpy, on the whole raster
        got, _ = A.decode_geotiff(m, data, level=1)
        assert np.array_equal(got.cpu().numpy().view(np.uint32), P.reduce(terrain).view(np.uint32))
        del got, dev
    side = n // 4
    with A.AerialGridMap(A.GridMapSettings(0.0, 0.0, side * 1.0, side * 1.0, 1.0), device=0) as m:
        for name, level in (("layer_level0", 0), ("layer_auto", -1)):
            out[name] = timed(lambda: A.layer_from_geotiff(m, "elevation", data, level=level), args.reps)
        auto = m.get("elevation")
        A.layer_from_geotiff(m, "elevation", data, level=2)
        assert np.array_equal(auto.view(np.uint32), m.get("elevation").view(np.uint32))
        out["auto_level"] = 2
    out["note"] = ("wall ms of synchronous calls; encode_*: raster in HBM -> file in HBM, its size read back; "
                   "the kernels' shares come from a kernel trace of --trace-target in a run of its own")
    line = json.dumps(out)
    print(line)
    path = args.out or os.path.join(ROOT, "profiles", "geotiff_pyramid_probe_%s.json" % hip_lib.build_id())
    with open(path, "w") as fh_:
        fh_.write(line + "\n")


if __name__ == "__main__":
    main()
