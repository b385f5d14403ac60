"""Developer tool: what the upscaled present (include/svr_upscale.h) costs on the MI355X, beside the scaled
svr_copy_to_swapchain it stands in for, and what a frame costs when it is rendered below the window's resolution.

Presents into a 3840x2160 R8G8B8A8 image, from a colour target of 1920x1080, 2560x1440 and 3840x2160 (identity):

    blit              svr_copy_to_swapchain (C16, LINEAR): the yardstick, from the same run
    upscale_plain     svr_upscale_to_swapchain with SVR_UPSCALE_NO_SHARPEN
    upscale_sharp     svr_upscale_to_swapchain, sharpness 0.5

Frames of bench.py's workload (configs[3], lod 1, 1024^2 textures), clear + geometry pass + present, in one run:

    native            3840x2160, svr_copy_to_swapchain at identity extent
    scale_0.5         render_extent(3840, 2160, 0.5) = 1920x1080, svr_upscale_to_swapchain (sharpness 0.5) to 3840x2160
    scale_0.667       render_extent(3840, 2160, 0.667) = 2561x1440, the same

Every figure is device time: two events on the contexts' stream around a window of --reps calls that starts from a fenced,
idle stream, divided by the calls.  The stages alternate inside every round, round 0 warms up, and the median, lowest and
highest window of the --rounds others are kept, so the run-to-run spread stands beside every figure.  No kernel's cost
depends on the values in the targets.  bytes/s come from one byte model for all three presents: the source's bytes once
(8 per RGBA16F texel) and the destination's once (4 per texel); taps shared between neighbouring outputs and tiles are
served by LDS and the caches and are not counted.

    python tools/upscaleprof.py [--reps 20] [--rounds 9] [--out profiles/upscale_cost.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402

DW, DH = 3840, 2160
RGBA = 1


def present_bytes(w, h):
    return 8 * w * h + 4 * DW * DH


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20, help="calls per timed window")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "upscale_cost.json"))
    args = ap.parse_args()
    pkg = g.load_package()
    import torch
    if not torch.cuda.is_available():
        sys.exit("upscaleprof: no GPU; these are device times and there is no fallback")
    S, A, M = pkg.scenes, pkg.abi, pkg.glmath
    lib = pkg.load_product_library()
    sc = S.sponza_like(lod=1, tex_size=1024)
    empty = np.zeros(0, A.RENDER_OBJECT_DTYPE)
    stream = torch.cuda.Stream()
    swap = torch.zeros((DH, DW, 4), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def context(w, h):
        """a context with the workload uploaded and one frame in its targets -> (renderer, draw)"""
        scene = S.scene_data_struct(*S.config3_camera(), w, h)
        r = lib.create(w, h)
        r.set_stream(stream.cuda_stream)
        opaque, _transparent = sc.render_objects(sc.upload(r))
        r.set_option(A.OPT_COUNT_FRAGMENTS, 0)

        def draw():
            r.clear_color((1, 1, 1, 1))
            r.draw_geometry(scene, opaque, empty)

        draw()
        r.sync()
        return r, draw

    def measure(stages):
        """stages: {name: (context, call)} -> {name: [ms per call of each kept window]}"""
        def window(r, call):
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
            for k, (r, call) in stages.items():
                t = window(r, call)
                if rnd:
                    ms[k].append(t)
        return ms

    def summary(samples, nbytes=None):
        a = np.array(samples)
        med = float(np.median(a))
        d = {"ms": round(med, 4), "min_ms": round(float(a.min()), 4), "max_ms": round(float(a.max()), 4),
             "spread_pct": round(100.0 * float(a.max() - a.min()) / med, 1)}
        if nbytes is not None:
            d["model_mb"] = round(nbytes / 1e6, 2)
            d["tb_per_s"] = round(nbytes / (med * 1e-3) / 1e12, 3)
        return d

    half = M.render_extent(DW, DH, 0.5)
    two_thirds = M.render_extent(DW, DH, 0.667)
    ctx = {ext: context(*ext) for ext in (half, (2560, 1440), two_thirds, (DW, DH))}
    presents = []
    for ext in (half, (2560, 1440), (DW, DH)):
        r = ctx[ext][0]
        stages = {"blit": (r, lambda r=r: r.copy_to_swapchain(swap.data_ptr(), DW, DH, RGBA)),
                  "upscale_plain": (r, lambda r=r: r.upscale_to_swapchain(swap.data_ptr(), DW, DH, RGBA, 0.5, A.UPSCALE_NO_SHARPEN)),
                  "upscale_sharp": (r, lambda r=r: r.upscale_to_swapchain(swap.data_ptr(), DW, DH, RGBA, 0.5, 0))}
        ms = measure(stages)
        out = {"source": list(ext), "destination": [DW, DH], "reps": args.reps, "rounds": args.rounds,
               "stages": {k: summary(v, present_bytes(*ext)) for k, v in ms.items()}}
        for k in ("upscale_plain", "upscale_sharp"):
            out[k + "_vs_blit"] = round(out["stages"][k]["ms"] / out["stages"]["blit"]["ms"], 3)
        print(json.dumps(out), flush=True)
        presents.append(out)

    def frame(ext, upscale):
        r, draw = ctx[ext]

        def call():
            draw()
            if upscale:
                r.upscale_to_swapchain(swap.data_ptr(), DW, DH, RGBA, 0.5, 0)
            else:
                r.copy_to_swapchain(swap.data_ptr(), DW, DH, RGBA)
        return r, call

    ms = measure({"native": frame((DW, DH), False), "scale_0.5": frame(half, True), "scale_0.667": frame(two_thirds, True)})
    frames = {"workload": "configs[3], lod 1, 1024^2 textures: clear, geometry pass, present into 3840x2160", "reps": args.reps, "rounds": args.rounds,
              "render_extent": {"native": [DW, DH], "scale_0.5": list(half), "scale_0.667": list(two_thirds)},
              "stages": {k: summary(v) for k, v in ms.items()}}
    for k in ("scale_0.5", "scale_0.667"):
        frames[k + "_vs_native"] = round(frames["stages"][k]["ms"] / frames["stages"]["native"]["ms"], 3)
    print(json.dumps(frames), flush=True)
    for r, _draw in ctx.values():
        r.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/upscaleprof.py", "device": torch.cuda.get_device_name(0), "presents": presents, "frames": frames}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
