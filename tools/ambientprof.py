"""Developer tool: what the ambient pass (include/svr_ambient.h) costs on the MI355X, on bench.py's workload (configs[3],
lod 1, 1024^2 textures) at 3840x2160 and 1920x1080, beside two yardsticks of the same run:

    the pass with its 5 x 5 blur                                  svr_ambient_pass
    the pass under SVR_AMBIENT_NO_BLUR (the second kernel copies)   svr_ambient_pass
    the lighting pass with 0 point lights, ambient factor on      svr_light_pass
    the lighting pass with 0 point lights, ambient factor off     svr_light_pass   (yardstick)
    the identity copy to an R8G8B8A8 swapchain image              svr_copy_to_swapchain   (yardstick)

Every figure is device time: two events on the context's stream around a window of --reps calls that starts from a fenced,
idle stream, divided by the calls.  The stages alternate inside every round, round 0 warms up, and the median, lowest and
highest window of the --rounds others are kept, so the run-to-run spread stands beside every figure.  The pass is out of
place, so every call does the same work.  bytes/s come from the byte models below, which count every byte a stage must
move once (the halo of a tile's window is re-read from the caches and not counted); the raw kernel is bound by its
arithmetic, not by these bytes, so its rate says how far from the memory roof it runs:

    copy       8 B read + 4 B written per pixel
    lighting   44 B per pixel (DESIGN.md §5 "Deferred lighting"), 48 B with the ambient factor
    ambient    raw kernel: depth 4 + normal 16 read, scratch 8 written = 28 B; blur kernel: scratch 8 read, target 4 written = 12 B

--only ambient runs the pass alone, a few calls: the run to put under rocprofv3 --kernel-trace.

    python tools/ambientprof.py [--reps 20] [--rounds 9] [--out profiles/ambient_cost.json]
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
LIGHT_AO_BYTES_PER_PIXEL = 48
COPY_BYTES_PER_PIXEL = 12
RAW_BYTES_PER_PIXEL = 4 + 16 + 8
BLUR_BYTES_PER_PIXEL = 8 + 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20, help="calls per timed window")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--sizes", default="3840x2160,1920x1080")
    ap.add_argument("--radius", type=float, default=0.5, help="world units")
    ap.add_argument("--only", default="", help="'ambient': a few calls of the pass and nothing else, no file written")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ambient_cost.json"))
    args = ap.parse_args()
    pkg = g.load_package()
    import torch
    if not torch.cuda.is_available():
        sys.exit("ambientprof: no GPU; these are device times and there is no fallback")
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
        _view, proj, vp = GL.scene_data(GL.camera_view(pos, pitch, yaw), w, h)[:3]
        m = np.asarray(vp, dtype=np.float64).T
        inv_vp = np.ascontiguousarray(np.linalg.inv(m).T.reshape(16), dtype=np.float32)
        ppu = GL.pixels_per_unit(proj, h)
        sun = (np.array(scene.ambient_color, np.float32), np.array(scene.sunlight_direction, np.float32), np.array(scene.sunlight_color, np.float32))
        swap = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")

        def ambient(flags=0):
            r.ambient_pass(inv_vp.reshape(4, 4), args.radius, ppu, 0.02 * args.radius, 1.0, 0.05, flags)

        def light(on):
            r.set_light_ambient_occlusion(on)
            r.light_pass(inv_vp, *sun)

        ambient()  # allocates the planes
        r.sync()
        ao = r.read_ambient()
        raw = r.read_ambient_raw()
        rpx = np.minimum(args.radius * float(ppu) * raw[..., 1], 16.0)
        picture = {"darkened_share": round(float((ao < 1).mean()), 4), "mean_factor": round(float(ao.mean()), 4),
                   "evaluated_share": round(float((rpx >= 1).mean()), 4), "capped_share": round(float((rpx >= 16).mean()), 4)}
        if args.only == "ambient":
            for _ in range(5):
                ambient()
                ambient(A.AMBIENT_NO_BLUR)
            r.sync()
            print(json.dumps({"width": w, "height": h, "picture": picture}), flush=True)
            r.close()
            continue

        px = w * h
        stages = {
            "ambient": (lambda: ambient(), (RAW_BYTES_PER_PIXEL + BLUR_BYTES_PER_PIXEL) * px),
            "ambient_no_blur": (lambda: ambient(A.AMBIENT_NO_BLUR), (RAW_BYTES_PER_PIXEL + BLUR_BYTES_PER_PIXEL) * px),
            "light_0_ao": (lambda: light(True), LIGHT_AO_BYTES_PER_PIXEL * px),
            "light_0": (lambda: light(False), LIGHT_BYTES_PER_PIXEL * px),
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
        out = {"width": w, "height": h, "reps": args.reps, "rounds": args.rounds, "radius": args.radius, "picture": picture, "stages": {},
               "ambient_bytes_by_kernel": {"ambient_raw_kernel": RAW_BYTES_PER_PIXEL * px, "ambient_blur_kernel": BLUR_BYTES_PER_PIXEL * px}}
        for k, (_call, nbytes) in stages.items():
            a = np.array(ms[k])
            med = float(np.median(a))
            out["stages"][k] = {"ms": round(med, 4), "min_ms": round(float(a.min()), 4), "max_ms": round(float(a.max()), 4),
                                "spread_pct": round(100.0 * float(a.max() - a.min()) / med, 1), "model_mb": round(nbytes / 1e6, 2),
                                "tb_per_s": round(nbytes / (med * 1e-3) / 1e12, 3)}
        st = out["stages"]
        out["blur_ms"] = round(st["ambient"]["ms"] - st["ambient_no_blur"]["ms"], 4)
        out["light_ao_extra_ms"] = round(st["light_0_ao"]["ms"] - st["light_0"]["ms"], 4)
        out["ns_per_pixel"] = round(st["ambient"]["ms"] * 1e6 / px, 4)
        print(json.dumps(out), flush=True)
        results.append(out)
        r.close()
    if args.only:
        return
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/ambientprof.py", "device": torch.cuda.get_device_name(0), "sizes": results}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
