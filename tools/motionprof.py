"""Developer tool: what the camera motion blur pass (include/svr_motion.h) costs on the MI355X beside the lighting pass, at
3840x2160 and 1920x1080, for four frames:

    the lighting pass with 0 point lights, the yardstick                   svr_light_pass          (bench.py's frame, configs[3])
    a still frame: every cell takes the skip path                          svr_motion_blur_pass    still
    the left half still, the right half moving 16 px                       svr_motion_blur_pass    half_16
    everything moving 8 px (16 taps) and 16 px (32 taps)                   svr_motion_blur_pass    full_8, full_16

Every figure is device time: two events on the contexts' stream around a window of --reps calls that starts from a fenced,
idle stream, divided by the calls.  The stages alternate inside every round, round 0 warms up, and the median, lowest and
highest window of the --rounds others are kept, so the run-to-run spread stands beside every figure.  The kernels' cost
depends on the velocities, which come from the depth image and the matrix alone (no branch reads a colour), so calling the
in-place pass again and again on its own output times the same work.  The depth images are synthetic and the reprojection
is affine in NDC, q.x = xn + (2 / W) z: a texel of depth 1 moves one pixel per unit of half the shutter, a texel of depth 0
is still.  Per-kernel times come from a separate
`rocprofv3 --kernel-trace --stats -- python tools/motionprof.py --rounds 1 --out /dev/null` run, not from here.

    python tools/motionprof.py [--reps 20] [--rounds 9] [--out profiles/motion_cost.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402

LIGHT_BYTES_PER_PIXEL = 44  # DESIGN.md §5 "Deferred lighting"


def motion_bytes(w, h):
    """bytes one pass must move once: the prepare reads colour and depth (12 B per pixel) and writes a prepared texel (16 B)
    and 8 B per cell; the gather reads the prepared image once (re-reads of the window's rim are the cache's), the old texel
    for its alpha (8 B) and writes colour (8 B)"""
    cells = ((w + 7) // 8) * ((h + 7) // 8)
    return {"motion_prepare_kernel": 28 * w * h + 8 * cells, "motion_gather_kernel": 32 * w * h + 8 * cells}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20, help="calls per timed window")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--sizes", default="3840x2160,1920x1080")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "motion_cost.json"))
    args = ap.parse_args()
    pkg = g.load_package()
    import torch
    if not torch.cuda.is_available():
        sys.exit("motionprof: no GPU; these are device times and there is no fallback")
    S, A = pkg.scenes, pkg.abi
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
        m = np.asarray(scene.viewproj, dtype=np.float64).reshape(4, 4).T
        inv_vp = np.ascontiguousarray(np.linalg.inv(m).T.reshape(16), dtype=np.float32)
        sun = (np.array(scene.ambient_color, np.float32), np.array(scene.sunlight_direction, np.float32), np.array(scene.sunlight_color, np.float32))

        # the depth images, each with a context of its own over caller tensors (one colour image serves all: seeded HDR)
        rng = np.random.default_rng(7)
        color = torch.from_numpy(np.ascontiguousarray((rng.uniform(0.0, 2.0, (h, w, 4)) ** 3).astype(np.float16)).view(np.int32)).cuda()  # [h, w, 2]
        still, moving = np.zeros((h, w), np.float32), np.ones((h, w), np.float32)
        half = still.copy()
        half[:, w // 2:] = 1.0
        reproject = np.eye(4, dtype=np.float32)  # [col][row]
        reproject[2][0] = np.float32(2.0 / w)
        images = {"still": (still, 32.0), "half_16": (half, 32.0), "full_8": (moving, 16.0), "full_16": (moving, 32.0)}  # (depth, shutter)
        keep, stages = [], {"light_0": lambda: r.light_pass(inv_vp, *sun)}
        for name, (depth, shutter) in images.items():
            d = torch.from_numpy(depth).cuda()
            rb = lib.create(w, h)
            rb.set_stream(stream.cuda_stream)
            rb.bind_targets(color.data_ptr(), d.data_ptr())
            keep.append((d, rb))
            stages[name] = (lambda rb=rb, shutter=shutter: rb.motion_blur_pass(reproject, shutter, 16.0))
        torch.cuda.synchronize()

        def window(call):
            r.sync()
            for _d, rb in keep:
                rb.sync()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(stream)
            for _ in range(args.reps):
                call()
            t1.record(stream)
            t1.synchronize()
            return t0.elapsed_time(t1) / args.reps

        ms = {k: [] for k in stages}
        for rnd in range(args.rounds + 1):  # round 0 warms up
            for k, call in stages.items():
                t = window(call)
                if rnd:
                    ms[k].append(t)
        out = {"width": w, "height": h, "reps": args.reps, "rounds": args.rounds, "max_blur": 16.0, "stages": {},
               "motion_bytes_by_kernel": motion_bytes(w, h), "light_model_mb": round(LIGHT_BYTES_PER_PIXEL * w * h / 1e6, 2)}
        for k in stages:
            a = np.array(ms[k])
            med = float(np.median(a))
            out["stages"][k] = {"ms": round(med, 4), "min_ms": round(float(a.min()), 4), "max_ms": round(float(a.max()), 4),
                                "spread_pct": round(100.0 * float(a.max() - a.min()) / med, 1)}
        for k in stages:
            if k != "light_0":
                out["stages"][k]["vs_light_0"] = round(out["stages"][k]["ms"] / out["stages"]["light_0"]["ms"], 3)
        print(json.dumps(out), flush=True)
        results.append(out)
        for _d, rb in keep:
            rb.close()
        r.close()
    if args.out != "/dev/null":
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"tool": "tools/motionprof.py", "device": torch.cuda.get_device_name(0), "sizes": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
