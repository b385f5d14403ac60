"""Developer tool: what the reflection pass (include/svr_reflect.h) costs on the MI355X beside the lighting pass, at
3840x2160, for these frames:

    the lighting pass with 0 point lights, the yardstick                   svr_light_pass          (bench.py's frame, configs[3])
    a frame of sky: nothing traces, every tile takes the empty path        svr_reflect_pass        sky
    the lower half floor, the upper half sky, 16 steps and 4 bisections    svr_reflect_pass        half_16_4
    a floor under a wall that fills the frame, 16 steps and 4 bisections
    and 64 and 8, each without and with the 3 x 3 resolve                  svr_reflect_pass        full_16_4_one, full_16_4, full_64_8_one, full_64_8

Every figure is device time: two events on the contexts' stream around a window of --reps calls that starts from a fenced,
idle stream, divided by the calls.  The stages alternate inside every round, round 0 warms up, and the median, lowest and
highest window of the --rounds others are kept, so the run-to-run spread stands beside every figure.  What a ray walks
depends on the depth, normal and albedo planes and the pass alone (the colour is read at a hit and by the composite; no
branch depends on it except the empty tile's "store what san changed"), so calling the in-place pass again and again on its
own output times the same work.  The G-buffers are tests/reflect_ref.py's analytic scenes, ray-cast on the host.  "walked"
is the mean number of samples a pixel of the frame evaluates, the bisections included, counted by a float64 march of the
same frame at a sixteenth of the extent each way (the figure an estimate is made from, not a check of the kernels).
Per-kernel times come from a separate
`rocprofv3 --kernel-trace --stats -- python tools/reflectprof.py --rounds 1 --out /dev/null` run, not from here.

    python tools/reflectprof.py [--reps 20] [--rounds 9] [--out profiles/reflect_cost.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as g  # noqa: E402
import reflect_ref as RR  # noqa: E402

LIGHT_BYTES_PER_PIXEL = 44  # DESIGN.md §5 "Deferred lighting"
PASS = dict(max_distance=14.3, thickness=0.1, f0=0.04, intensity=1.0, distance_fade=1.0, edge_width=16.0, depth_tolerance=0.05, frame_index=0)


def reflect_bytes(w, h):
    """bytes one pass must move once where every pixel traces: the trace reads depth (4 B), the albedo flag's line and the
    normal (16 B each) and writes a trace texel (16 B); the resolve reads the trace texels (16 B), depth (4 B) and colour (8 B)
    and writes colour (8 B).  The march's depth texels and the hits' colour texels are the cache's"""
    return {"reflect_trace_kernel": 52 * w * h, "reflect_resolve_kernel": 36 * w * h}


def frames(w, h):
    """name -> (camera, G-buffer)"""
    level = RR.Camera(w, h, eye=(0.3, 1.6, 2.0), target=(0.3, 1.6, -6.0), fov_y=0.8)   # the horizon through the middle
    down = RR.Camera(w, h, eye=(0.3, 2.6, 2.0), target=(0.0, 0.4, -4.0), fov_y=0.8)
    sky = RR.cast(level, wall_z=-1000.0, wall_h=0.0, box=None)  # a floor to the horizon, no wall
    half = {k: v.copy() for k, v in sky.items()}
    for k in ("depth", "normal", "albedo"):
        sky[k][...] = 0
    return {"sky": (level, sky), "half": (level, half), "full": (down, RR.cast(down, wall_h=100.0, box=None))}


def walked(cam, g, steps, refine, **kw):
    """the mean number of samples a pixel of g evaluates: trace64's count over every pixel, those that trace nothing too"""
    m = RR.trace64(g, *cam.args(), **dict(kw, steps=steps, refine=refine))
    return float(m["samples"].mean()), float((m["hit"][..., 0] >= 0).mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20, help="calls per timed window")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--sizes", default="3840x2160")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reflect_cost.json"))
    args = ap.parse_args()
    pkg = g.load_package()
    import torch
    if not torch.cuda.is_available():
        sys.exit("reflectprof: no GPU; these are device times and there is no fallback")
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

        # a context of its own per frame over caller tensors (one colour image serves all: seeded HDR)
        rng = np.random.default_rng(7)
        color = torch.from_numpy(np.ascontiguousarray((rng.uniform(0.0, 2.0, (h, w, 4)) ** 3).astype(np.float16)).view(np.int32)).cuda()  # [h, w, 2]
        keep, stages, counts = {}, {"light_0": lambda: r.light_pass(inv_vp, *sun)}, {}
        small = frames(w // 16, h // 16)
        for name, (cam, gb) in frames(w, h).items():
            planes = [torch.from_numpy(np.ascontiguousarray(gb[k])).cuda() for k in ("depth", "normal", "albedo")]
            rb = lib.create(w, h)
            rb.set_stream(stream.cuda_stream)
            rb.bind_targets(color.data_ptr(), planes[0].data_ptr())
            rb.bind_attribute_target(A.ATTR_NORMAL, planes[1].data_ptr())
            rb.bind_attribute_target(A.ATTR_ALBEDO, planes[2].data_ptr())
            keep[name] = (planes, rb, cam)
        del gb

        def stage(frame, steps, refine, resolve):
            _planes, rb, cam = keep[frame]
            return lambda: rb.reflect_pass(*cam.args(), steps=steps, refine=refine, resolve=resolve, **PASS)

        stages["sky"] = stage("sky", 16, 4, 1)
        stages["half_16_4"] = stage("half", 16, 4, 1)
        for steps, refine in ((16, 4), (64, 8)):
            stages[f"full_{steps}_{refine}_one"] = stage("full", steps, refine, 0)
            stages[f"full_{steps}_{refine}"] = stage("full", steps, refine, 1)
        counts["sky"] = walked(*small["sky"], 16, 4, **PASS)
        counts["half_16_4"] = walked(*small["half"], 16, 4, **PASS)
        for steps, refine in ((16, 4), (64, 8)):
            counts[f"full_{steps}_{refine}"] = counts[f"full_{steps}_{refine}_one"] = walked(*small["full"], steps, refine, **PASS)
        torch.cuda.synchronize()

        def window(call):
            r.sync()
            for _planes, rb, _cam in keep.values():
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
        out = {"width": w, "height": h, "reps": args.reps, "rounds": args.rounds, "pass": PASS, "stages": {},
               "reflect_bytes_by_kernel": reflect_bytes(w, h), "light_model_mb": round(LIGHT_BYTES_PER_PIXEL * w * h / 1e6, 2)}
        for k in stages:
            a = np.array(ms[k])
            med = float(np.median(a))
            out["stages"][k] = {"ms": round(med, 4), "min_ms": round(float(a.min()), 4), "max_ms": round(float(a.max()), 4),
                                "spread_pct": round(100.0 * float(a.max() - a.min()) / med, 1)}
        for k in stages:
            if k != "light_0":
                out["stages"][k]["vs_light_0"] = round(out["stages"][k]["ms"] / out["stages"]["light_0"]["ms"], 3)
                out["stages"][k]["walked_per_pixel"], out["stages"][k]["hit_share"] = (round(v, 3) for v in counts[k])
        print(json.dumps(out), flush=True)
        results.append(out)
        for _planes, rb, _cam in keep.values():
            rb.close()
        r.close()
    if args.out != "/dev/null":
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"tool": "tools/reflectprof.py", "device": torch.cuda.get_device_name(0), "sizes": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
