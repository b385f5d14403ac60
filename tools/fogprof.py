"""Developer tool: what the fog pass (include/svr_fog.h) costs on the MI355X beside the lighting pass, on bench.py's workload
(configs[3], lod 1, 1024^2 textures) at 3840x2160 and 1920x1080:

    the lighting pass with 0 point lights, the yardstick             svr_light_pass
    the fog pass with 16 and with 32 steps, without a shadow map     svr_fog_pass
    the same with a 1024 x 1024 shadow map drawn from above           svr_fog_pass

Every figure is device time: two events on the context's stream around a window of --reps calls that starts from a fenced,
idle stream, divided by the calls.  The stages alternate inside every round, round 0 warms up, and the median, lowest and
highest window of the --rounds others are kept, so the run-to-run spread stands beside every figure.  The kernels' cost does
not depend on the values in the colour target (no branch of them does), so calling the in-place pass again and again on its
own output times the same work; the depth target, which decides every ray's length, is the frame's and does not change.
The shadow map is synthetic: an orthographic light straight above the atrium whose texels hold seeded slab heights, so
neighbouring rays read neighbouring texels as they would in a drawn map.  Per-kernel times come from a separate
`rocprofv3 --kernel-trace --stats -- python tools/fogprof.py --rounds 1 --out /dev/null` run, not from here.

    python tools/fogprof.py [--reps 20] [--rounds 9] [--out profiles/fog_cost.json]
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
MAP = 1024


def fog_bytes(w, h):
    """bytes one fog pass must move once: the march reads depth (4 B per pixel) and writes 20 B per block; the composite
    reads depth and colour and writes colour (20 B per pixel) and reads the blocks once (re-reads are the LDS's)"""
    blocks = ((w + 1) // 2) * ((h + 1) // 2)
    return {"fog_march_kernel": 4 * w * h + 20 * blocks, "fog_composite_kernel": 20 * w * h + 20 * blocks}


def light_from_above(center, half, height):
    """column-major viewproj of an orthographic light looking straight down on a (2 half)^2 square around center"""
    cx, cy, cz = center
    top = cy + 0.5 * height
    M = np.array([[1 / half, 0, 0, -cx / half], [0, 0, 1 / half, -cz / half], [0, 1 / height, 0, 1 - top / height], [0, 0, 0, 1]], np.float64)
    return M, np.ascontiguousarray(M.T.reshape(16), dtype=np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20, help="calls per timed window")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--sizes", default="3840x2160,1920x1080")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fog_cost.json"))
    args = ap.parse_args()
    pkg = g.load_package()
    import torch
    if not torch.cuda.is_available():
        sys.exit("fogprof: no GPU; these are device times and there is no fallback")
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
        eye = np.asarray(pos, np.float64)
        M, light_vp = light_from_above((eye[0], eye[1], eye[2]), half=120.0, height=240.0)
        rng = np.random.default_rng(7)
        slabs = M[2, 1] * (eye[1] + rng.uniform(2.0, 30.0, (MAP // 16, MAP // 16))) + M[2, 3]
        slabs[rng.random(slabs.shape) < 0.5] = 0.0
        smap = torch.from_numpy(np.kron(slabs, np.ones((16, 16))).astype(np.float32)).cuda()
        torch.cuda.synchronize()
        fog = dict(density=0.02, height_falloff=0.05, height_base=float(eye[1]), max_distance=150.0, fog_color=(0.5, 0.6, 0.7),
                   sun_dir=(0.0, 1.0, 0.0, 0.0), sun_color=(4.0, 3.5, 3.0), anisotropy=0.5, edge_sharpness=1.0)
        shadow = dict(shadow_ptr=smap.data_ptr(), shadow_size=(MAP, MAP), shadow_viewproj=light_vp, shadow_bias=0.002)
        frame = [0]

        def fog_call(steps, with_map):
            def call():
                frame[0] += 1
                r.fog_pass(inv_vp, eye, steps=steps, frame_index=frame[0], **fog, **(shadow if with_map else {}))
            return call

        stages = {"light_0": lambda: r.light_pass(inv_vp, *sun)}
        for steps in (16, 32):
            for with_map in (False, True):
                stages[f"fog_{steps}{'_map' if with_map else ''}"] = fog_call(steps, with_map)

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
            for k, call in stages.items():
                t = window(call)
                if rnd:
                    ms[k].append(t)
        out = {"width": w, "height": h, "reps": args.reps, "rounds": args.rounds, "stages": {}, "fog_bytes_by_kernel": fog_bytes(w, h),
               "light_model_mb": round(LIGHT_BYTES_PER_PIXEL * w * h / 1e6, 2)}
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
        r.close()
    if args.out != "/dev/null":
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"tool": "tools/fogprof.py", "device": torch.cuda.get_device_name(0), "sizes": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
