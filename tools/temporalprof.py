"""Developer tool: what temporal antialiasing (include/svr_temporal.h) costs on the MI355X, on bench.py's workload
(configs[3], lod 1, 1024^2 textures) at 3840x2160 and 1920x1080, beside two yardsticks of the same run:

    the resolve under a small yaw step (nearly every pixel uses the history)   svr_temporal_resolve
    the resolve under SVR_TEMPORAL_RESET (no history tap is fetched)           svr_temporal_resolve
    the lighting pass with 0 point lights                                      svr_light_pass
    the identity copy to an R8G8B8A8 swapchain image                           svr_copy_to_swapchain

Every figure is device time: two events on the context's stream around a window of --reps calls that starts from a fenced,
idle stream, divided by the calls.  The stages alternate inside every round, round 0 warms up, and the median, lowest and
highest window of the --rounds others are kept, so the run-to-run spread stands beside every figure.  No branch of the
kernels depends on the colour values, and the depth target and the matrix (which decide where the history is fetched) stay
the same, so calling the in-place pass again and again on its own output times the same work.  bytes/s come from the byte
models below, which count every byte a stage must move once:

    copy      8 B read + 4 B written per pixel
    lighting  44 B per pixel (DESIGN.md §5 "Deferred lighting": depth 4, normal 16, albedo 16, colour 8)
    temporal  resolve kernel: colour 8 + depth 4 read, history 8 read (one texel per pixel: the four taps of neighbouring
              pixels overlap and are served by the caches; 0 under RESET), new history 8 written;
              copy kernel: new history 8 + colour 8 read (the alpha half is kept), colour 8 written.
              The one-texel halo of a tile's window is re-read from the caches and not counted.

    python tools/temporalprof.py [--reps 20] [--rounds 9] [--out profiles/temporal_cost.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402

LIGHT_BYTES_PER_PIXEL = 44
COPY_BYTES_PER_PIXEL = 12
RESOLVE_BYTES_PER_PIXEL = 8 + 4 + 8 + 8
RESOLVE_RESET_BYTES_PER_PIXEL = 8 + 4 + 8
HISTORY_COPY_BYTES_PER_PIXEL = 8 + 8 + 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20, help="calls per timed window")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--sizes", default="3840x2160,1920x1080")
    ap.add_argument("--yaw-step", type=float, default=0.01, help="radians between the two cameras of the reprojection")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal_cost.json"))
    args = ap.parse_args()
    pkg = g.load_package()
    import torch
    if not torch.cuda.is_available():
        sys.exit("temporalprof: no GPU; these are device times and there is no fallback")
    S, A, GL = pkg.scenes, pkg.abi, pkg.glmath
    lib = pkg.load_product_library()
    sc = S.sponza_like(lod=1, tex_size=1024)
    empty = np.zeros(0, A.RENDER_OBJECT_DTYPE)
    stream = torch.cuda.Stream()
    results = []
    for size in args.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        pos, pitch, yaw = S.config3_camera()
        scene = S.scene_data_struct(pos, pitch, yaw, w, h)
        r = lib.create(w, h)
        r.set_stream(stream.cuda_stream)
        opaque, _transparent = sc.render_objects(sc.upload(r))
        r.set_option(A.OPT_COUNT_FRAGMENTS, 0)
        r.enable_attributes(A.ATTR_NORMAL | A.ATTR_ALBEDO)
        r.clear_color((1, 1, 1, 1))
        r.draw_geometry(scene, opaque, empty)
        vp = GL.scene_data(GL.camera_view(pos, pitch, yaw), w, h)[2]
        prev = GL.scene_data(GL.camera_view(pos, pitch, yaw - args.yaw_step), w, h)[2]
        reproject = GL.temporal_reproject(prev, vp)
        m = np.asarray(vp, dtype=np.float64).T
        inv_vp = np.ascontiguousarray(np.linalg.inv(m).T.reshape(16), dtype=np.float32)
        sun = (np.array(scene.ambient_color, np.float32), np.array(scene.sunlight_direction, np.float32), np.array(scene.sunlight_color, np.float32))
        swap = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
        r.temporal_resolve(reproject, 0.1)  # allocates the history; every later call finds it valid
        torch.cuda.synchronize()

        px = w * h
        stages = {
            "temporal": (lambda: r.temporal_resolve(reproject, 0.1), (RESOLVE_BYTES_PER_PIXEL + HISTORY_COPY_BYTES_PER_PIXEL) * px),
            "temporal_reset": (lambda: r.temporal_resolve(reproject, 0.1, A.TEMPORAL_RESET), (RESOLVE_RESET_BYTES_PER_PIXEL + HISTORY_COPY_BYTES_PER_PIXEL) * px),
            "light_0": (lambda: r.light_pass(inv_vp, *sun), LIGHT_BYTES_PER_PIXEL * px),
            "copy_identity": (lambda: r.copy_to_swapchain(swap.data_ptr(), w, h, 0), COPY_BYTES_PER_PIXEL * px),
        }

        def window(call):
            r.sync()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(stream)
            for _ in range(args.reps):
                call()
            t1.record(stream)
            t1.synchronize()
            r.sync()
            return t0.elapsed_time(t1) / args.reps

        ms = {k: [] for k in stages}
        for rnd in range(args.rounds + 1):  # round 0 warms up
            for k, (call, _b) in stages.items():
                t = window(call)
                if rnd:
                    ms[k].append(t)
        out = {"width": w, "height": h, "reps": args.reps, "rounds": args.rounds, "yaw_step": args.yaw_step, "stages": {},
               "temporal_bytes_by_kernel": {"temporal_resolve_kernel": RESOLVE_BYTES_PER_PIXEL * px, "temporal_copy_kernel": HISTORY_COPY_BYTES_PER_PIXEL * px}}
        for k, (_call, nbytes) in stages.items():
            a = np.array(ms[k])
            med = float(np.median(a))
            out["stages"][k] = {"ms": round(med, 4), "min_ms": round(float(a.min()), 4), "max_ms": round(float(a.max()), 4),
                                "spread_pct": round(100.0 * float(a.max() - a.min()) / med, 1), "model_mb": round(nbytes / 1e6, 2),
                                "tb_per_s": round(nbytes / (med * 1e-3) / 1e12, 3)}
        out["temporal_vs_copy_rate"] = round(out["stages"]["temporal"]["tb_per_s"] / out["stages"]["copy_identity"]["tb_per_s"], 3)
        out["temporal_vs_light_rate"] = round(out["stages"]["temporal"]["tb_per_s"] / out["stages"]["light_0"]["tb_per_s"], 3)
        print(json.dumps(out), flush=True)
        results.append(out)
        r.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/temporalprof.py", "device": torch.cuda.get_device_name(0), "sizes": results}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
