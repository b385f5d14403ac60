"""Developer tool: occlusion culling (include/svr_occlusion.h) against the same frame without it, at the shapes of DESIGN
section 5 (occlusion culling).

    python tools/occlprof.py [--frames 50] [--rounds 5] [--only 4k,8k_x16] [--mode off,last,prepass]

Shapes: configs[3] at 3840x2160 (4k) and configs[4] x16 at 7680x4320 (8k_x16), with bench.py's textures (25 x 1024^2).
Per frame: svr_clear_color + svr_draw_geometry over the opaque and transparent objects, with
  off      no pyramid bound;
  last     culling against the pyramid of the previous frame's depth (a build behind every frame);
  prepass  a depth-only pass of the occluders (the quarter of the opaque objects with the most triangles: the atrium's
           floors, walls and colonnades), a build, then the frame culling against it.
The modes alternate in fenced windows of --frames frames; frame time = device events around the window / frames.
Medians over --rounds windows.  Then one instrumented frame per mode for the culled share of chunks and triangles, and
the build alone (--frames builds of the context's depth) for its time and its share of the HBM roofline.  The kernel
split: one shape and one mode at a time under
`rocprofv3 --kernel-trace --stats -- python tools/occlprof.py --only 4k --mode last`.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402

SHAPES = ("4k", "8k_x16")
MODES = ("off", "last", "prepass")
HBM_TBPS = 8.0  # MI355X HBM3E peak, datasheet


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", default="", help="comma-separated shapes of " + ", ".join(SHAPES))
    ap.add_argument("--mode", default=",".join(MODES))
    ap.add_argument("--tex", type=int, default=1024)
    args = ap.parse_args()
    import torch
    pkg = g.load_package()
    S, A = pkg.scenes, pkg.abi
    hip = pkg.load_product_library()
    only = [s for s in args.only.split(",") if s]
    modes = [m for m in args.mode.split(",") if m]
    for shape in SHAPES:
        if only and shape not in only:
            continue
        w, h = (7680, 4320) if shape == "8k_x16" else (3840, 2160)
        sc = S.sponza_like(lod=1, tex_size=args.tex)
        r = hip.create(w, h)
        inst = S.config5_instances() if shape == "8k_x16" else None
        opaque, transparent = sc.render_objects(sc.upload(r), instance_transforms=inst)
        pos, pitch, yaw = S.config5_camera() if shape == "8k_x16" else S.config3_camera()
        scene = S.scene_data_struct(pos, pitch, yaw, w, h)
        order = np.argsort(-opaque["index_count"].astype(np.int64), kind="stable")
        occluders = opaque[np.sort(order[:max(1, len(opaque) // 4)])]
        pyr = r.create_depth_pyramid()
        white = (1.0, 1.0, 1.0, 1.0)

        def frame(mode):
            if mode == "prepass":
                r.set_occlusion_pyramid(0)
                r.draw_depth(scene, occluders)
                r.build_depth_pyramid(pyr)
            r.set_occlusion_pyramid(0 if mode == "off" else pyr)
            r.clear_color(white)
            r.draw_geometry(scene, opaque, transparent)
            if mode == "last":
                r.build_depth_pyramid(pyr)

        for m in modes:  # warm-up (and "last" gets its first pyramid)
            for _ in range(5):
                frame(m)
        r.sync()
        res = {m: [] for m in modes}
        for _ in range(args.rounds):
            for m in modes:
                if m == "last":
                    frame("last")
                r.sync()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.frames):
                    frame(m)
                r.sync()
                e1.record()
                e1.synchronize()
                res[m].append(e0.elapsed_time(e1) / args.frames * 1e3)
        out = {"shape": shape, "width": w, "height": h, "occluders": int(len(occluders)), "objects": int(len(opaque))}
        r.set_option(A.OPT_COUNT_FRAGMENTS, 1)
        for m in modes:
            frame(m)
            if m == "last":
                frame(m)
            r.sync()
            o, st = r.occlusion_stats(), r.get_stats()
            out[m] = {"frame_us": round(float(np.median(res[m])), 1), "chunks_tested": int(o.chunks_tested),
                      "chunks_culled": int(o.chunks_culled), "triangles_culled": int(o.triangles_culled),
                      "triangle_share": round(o.triangles_culled / max(1, st.triangle_count), 3),
                      "binned_triangles": int(st.binned_triangles)}
        r.set_option(A.OPT_COUNT_FRAGMENTS, 0)
        # the build alone
        r.sync()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.frames):
            r.build_depth_pyramid(pyr)
        r.sync()
        e1.record()
        e1.synchronize()
        us = e0.elapsed_time(e1) / args.frames * 1e3
        moved = w * h * 4 * (1 + 1 / 3)  # read level 0, write levels 1.. (a third of it)
        out["build_us"] = round(us, 1)
        out["build_gbps"] = round(moved / us / 1e3, 1)
        out["build_roofline_share"] = round(moved / us / 1e6 / HBM_TBPS, 3)
        r.close()
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
