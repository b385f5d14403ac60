"""Developer tool: depth-only passes (include/svr_depth.h) against the full pass they stand in for, at the shapes of
DESIGN section 5 (depth-only passes).

    python tools/depthprof.py [--frames 50] [--rounds 5] [--only 4k,8k_x16] [--lib build_ab/libsvr_hip_X.so] [--tuning N]

Shapes: configs[3] at 3840x2160 without and with an ID target (4k, 4k_ids), configs[4] x16 at 7680x4320 (8k_x16), all
with bench.py's textures (25 x 1024^2), and the atrium as six 512 x 512 cube faces through the list-views path (cube6).
The full pass is svr_clear_color + svr_draw_geometry over the opaque and transparent objects (cube6: svr_draw_list_views
with clear_rgba); the depth-only pass is svr_draw_depth over the opaque ones (cube6: svr_draw_list_depth_views).  The
two are alternated in fenced windows of --frames passes; frame time = device events around the window / frames, host
time = the library's own time inside the calls (SvrStats.mesh_draw_time), also with every pass fenced ("fenced host":
an idle GPU).  Medians over --rounds windows.  The kernel-trace split: one shape and one path at a time under
`rocprofv3 --kernel-trace --stats -- python tools/depthprof.py --only 4k --path depth`.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402

SHAPES = ("4k", "4k_ids", "8k_x16", "cube6")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", default="", help="comma-separated shapes of " + ", ".join(SHAPES))
    ap.add_argument("--path", default="both", choices=("both", "full", "depth"))
    ap.add_argument("--lib", default="", help="another build of libsvr_hip.so (tools/build_variant.sh)")
    ap.add_argument("--tuning", type=int, default=0, help="SVR_OPT_TUNING for both paths")
    args = ap.parse_args()
    import torch
    pkg = g.load_package()
    S, GM, A = pkg.scenes, pkg.glmath, pkg.abi
    hip = A.SvrLib(args.lib) if args.lib else pkg.load_product_library()
    only = [s for s in args.only.split(",") if s]
    for shape in SHAPES:
        if only and shape not in only:
            continue
        white = (1.0, 1.0, 1.0, 1.0)
        keep = []
        if shape == "cube6":
            w = h = 512
            sc = S.sponza_like(lod=1, tex_size=64)
            r = hip.create(w, h)
            opaque, transparent = sc.render_objects(sc.upload(r))
            pos = (0.0, 2.0, 0.0)
            faces = [(0.0, 0.0), (0.0, 90.0), (0.0, 180.0), (0.0, 270.0), (89.0, 0.0), (-89.0, 0.0)]
            scenes = [S.scene_data_struct(pos, np.float32(GM.radians(p)), np.float32(GM.radians(y)), w, h) for p, y in faces]
            lst = r.create_draw_list(opaque, transparent)
            color = torch.zeros((6, h, w, 4), dtype=torch.int16, device="cuda")
            depth = torch.zeros((6, h, w), dtype=torch.float32, device="cuda")
            keep += [color, depth, lst]

            def full():
                return r.draw_list_views(scenes, lst, color.data_ptr(), depth.data_ptr(), clear_rgba=white).mesh_draw_time

            def dep():
                return r.draw_list_depth_views(scenes, lst, depth.data_ptr()).mesh_draw_time
        else:
            w, h = (7680, 4320) if shape == "8k_x16" else (3840, 2160)
            sc = S.sponza_like(lod=1, tex_size=1024)
            r = hip.create(w, h)
            inst = S.config5_instances() if shape == "8k_x16" else None
            opaque, transparent = sc.render_objects(sc.upload(r), instance_transforms=inst)
            pos, pitch, yaw = S.config5_camera() if shape == "8k_x16" else S.config3_camera()
            scene = S.scene_data_struct(pos, pitch, yaw, w, h)
            if shape == "4k_ids":
                r.enable_ids()

            def full():
                r.clear_color(white)
                return r.draw_geometry(scene, opaque, transparent).mesh_draw_time

            def dep():
                return r.draw_depth(scene, opaque).mesh_draw_time
        r.set_option(A.OPT_TUNING, args.tuning)
        paths = {"full": full, "depth": dep}
        if args.path != "both":
            paths = {args.path: paths[args.path]}
        for f in paths.values():  # warm-up
            for _ in range(5):
                f()
        r.sync()
        res = {p: ([], [], []) for p in paths}
        for _ in range(args.rounds):
            for p, f in paths.items():
                r.sync()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                host_ms = 0.0
                for _ in range(args.frames):
                    host_ms += f()
                r.sync()
                e1.record()
                e1.synchronize()
                res[p][0].append(e0.elapsed_time(e1) / args.frames * 1e3)
                res[p][1].append(host_ms / args.frames * 1e3)
                fenced = 0.0
                for _ in range(min(args.frames, 20)):
                    fenced += f()
                    r.sync()
                res[p][2].append(fenced / min(args.frames, 20) * 1e3)
        for o in keep[2:]:
            o.close()
        r.close()
        out = {"shape": shape, "width": w, "height": h, "tuning": args.tuning, "lib": os.path.basename(args.lib) or "libsvr_hip.so"}
        for p, (fr, ho, fe) in res.items():
            out[p] = {"frame_us": round(float(np.median(fr)), 1), "host_us": round(float(np.median(ho)), 1),
                      "fenced_host_us": round(float(np.median(fe)), 1)}
        if len(res) == 2:
            out["depth_over_full"] = round(out["depth"]["frame_us"] / out["full"]["frame_us"], 3)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
