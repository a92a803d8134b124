"""One JSON line: what writing a map layer / a mosaic as JPEG costs on one MI355X, next to what the
library did before for the same image (the 8-bit raster downloaded and written raw).  3 warm-up and
20 timed repeats each, median and interquartile range, plus the library's build id.
  * the 10 000 x 10 000 gray `ortho` layer of cfg3's map (2500 m at 0.25 m; synthetic texture)
  * a 1000 x 1000 colour mosaic (synthetic frames through OrthoForwardHomography.batch)
Columns: encode_dev (amhip_jpeg_encode_dev / amhip_mosaic_encode_jpeg_dev: wall ms of the call, and
the HIP-event ms of the AMHIP_K_MISC slot, which times the encoder's kernels as one region -- the slot
cannot split them), write (encode + download + file),
raw (amhip_layer_to_image / amhip_mosaic_download + the raster written with tofile), pillow
(Image.save of the same image in memory, where Pillow is installed).
The result also goes to profiles/jpeg_probe_<build id>.json (--out FILE: elsewhere).
The per-kernel split comes from a kernel trace of a fresh process that only encodes the layer:
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- python tools/jpeg_probe.py --trace-target
(its *_kernel_stats.csv lists the k_jpeg_* kernels; DESIGN 4.10 quotes it).
Usage: python tools/jpeg_probe.py [--reps N] [--size N] [--out FILE] [--trace-target]"""
import argparse
import ctypes as C
import io
import json
import os
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
    ap.add_argument("--size", type=int, default=10000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-target", action="store_true",
                    help="only encode the layer image five times (the program to run under a kernel trace)")
    args = ap.parse_args()
    import numpy as np
    import torch
    import aerial_mapper_amd as A
    from aerial_mapper_amd import export as E, hip_lib, synth
    try:
        from PIL import Image
    except ImportError:
        Image = None
    lib = hip_lib.load()
    out = {"build_id": hip_lib.build_id(), "reps": args.reps, "warmup": 3, "layer": {}, "mosaic": {},
           "pillow": "measured" if Image else "not available"}
    tmp = tempfile.mkdtemp(prefix="jpeg_probe")

    def pillow_ms(img):
        def run():
            im = Image.fromarray(img if img.ndim == 2 else np.ascontiguousarray(img[..., ::-1]))
            im.save(io.BytesIO(), "JPEG", quality=95, subsampling=2, optimize=False)
        return timed(run, 3, warm=1)

    # ---- the map layer ----
    n, res = args.size, 0.25
    with A.AerialGridMap(A.GridMapSettings(0.0, 0.0, n * res, n * res, res), device=0) as m:
        tile = synth.make_frames(1, 1000, 1000, 1, salt=3)[0].astype(np.float32)
        layer = np.tile(tile, ((n + 999) // 1000, (n + 999) // 1000))[:n, :n]
        layer += (np.arange(n, dtype=np.float32) % 7)[None, :]     # (no two tiles alike)
        m.set("ortho", np.ascontiguousarray(layer))
        del layer
        img_dev = torch.empty((n, n), dtype=torch.uint8, device="cuda")
        hip_lib.check(lib.amhip_layer_to_image_dev(m._h, 0, 0, 0.0, 255.0, C.c_void_p(img_dev.data_ptr()), n))
        m.synchronize()
        dev_out = torch.empty(lib.amhip_jpeg_bound(n, n, 1), dtype=torch.uint8, device="cuda")
        nbytes = C.c_size_t()

        def encode_dev():
            hip_lib.check(lib.amhip_jpeg_encode_dev(m._h, C.c_void_p(img_dev.data_ptr()), n, n, n, 1, 95,
                                                    C.c_void_p(dev_out.data_ptr()), dev_out.numel(),
                                                    C.byref(nbytes)))
        if args.trace_target:
            for _ in range(5):
                encode_dev()
            print(json.dumps({"trace_target": True, "file_bytes": int(nbytes.value), "build_id": hip_lib.build_id()}))
            return
        r = timed(encode_dev, args.reps)
        m.enable_timing(True)
        m.timing_reset()
        encode_dev()
        m.synchronize()
        r["k_misc_event_ms"] = m.kernel_times()[lib.amhip_kernel_name(hip_lib.K_MISC).decode()][0]
        m.enable_timing(False)
        out["layer"]["encode_dev"] = r
        out["layer"]["file_bytes"] = int(nbytes.value)
        out["layer"]["pixels"] = n * n
        f = os.path.join(tmp, "layer.jpg")
        out["layer"]["write"] = timed(lambda: E.layer_to_jpeg(m, "ortho", f, 0.0, 255.0), args.reps)
        raw = os.path.join(tmp, "layer.raw")
        out["layer"]["raw"] = timed(lambda: E.layer_to_image(m, "ortho", 0.0, 255.0).tofile(raw), args.reps)
        out["layer"]["raw_bytes"] = n * n
        if Image:
            out["layer"]["pillow"] = pillow_ms(E.layer_to_image(m, "ortho", 0.0, 255.0))
        del img_dev, dev_out
    # ---- the mosaic ----
    W = H = 1000
    fw, fh = 320, 240
    ncam = A.NCamera(250.0, 250.0, (fw - 1) / 2.0, (fh - 1) / 2.0, fw, fh)
    st = A.OrthoForwardHomographySettings(ground_plane_elevation_m=400.0, width_mosaic_pixels=W,
                                          height_mosaic_pixels=H)
    poses = synth.make_lawnmower_poses(24, 400.0, 520.0, 5, tilt_deg=3.0)
    frames = synth.make_frames(24, fh, fw, 3, salt=11)
    with A.OrthoForwardHomography(ncam, st) as mosaic:
        mosaic.batch(poses, [f for f in frames])
        out["mosaic"]["covered"] = float((mosaic.result()[1] > 0).mean())
        out["mosaic"]["encode_dev"] = timed(lambda: mosaic.encode_jpeg(95), args.reps)
        f = os.path.join(tmp, "mosaic.jpg")
        out["mosaic"]["write"] = timed(lambda: mosaic.write_jpeg(f, 95), args.reps)
        out["mosaic"]["file_bytes"] = os.path.getsize(f)
        raw = os.path.join(tmp, "mosaic.raw")
        out["mosaic"]["raw"] = timed(lambda: mosaic.result()[0].tofile(raw), args.reps)
        out["mosaic"]["raw_bytes"] = W * H * 3 * 2
        if Image:
            out["mosaic"]["pillow"] = pillow_ms(np.clip(mosaic.result()[0], 0, 255).astype(np.uint8))
    out["note"] = ("wall ms of synchronous calls; encode_dev of the mosaic includes the bytes' download "
                   "(Python's encode_jpeg returns them); k_misc_event_ms: HIP events around the "
                   "encoder's kernels, one region")
    line = json.dumps(out)
    print(line)
    path = args.out or os.path.join(ROOT, "profiles", "jpeg_probe_%s.json" % hip_lib.build_id())
    with open(path, "w") as fh_:
        fh_.write(line + "\n")


if __name__ == "__main__":
    main()
