"""Developer tool: K views drawn by one multiview pass (include/svr_views.h) against K single-view passes, on the atrium
of configs[3] drawn from a retained draw list, at the three shapes of DESIGN section 5.

    python tools/viewprof.py [--frames 100] [--rounds 5] [--only 6x512x512]

A frame is K views into the layers of one pair of device targets [K, H, W, C] with a clear: K x (svr_clear_color +
svr_draw_list into layer k, bound with svr_bind_targets) against one svr_draw_list_views with clear_rgba.  The two are
alternated in fenced windows of --frames frames (svr_sync on both sides); frame time = device events around the
window / frames, host time = the library's own time inside the calls (SvrStats.mesh_draw_time) per frame.  In those
pipelined windows the host time includes waits for a free operation-log slot (eight operations in flight), so it is
also measured with every frame fenced (svr_sync behind it: an idle GPU, as tools/listprof.py does): "fenced host".
Medians over --rounds windows.  The kernel-trace split: run one shape and one path at a time under
`rocprofv3 --kernel-trace --stats -- python tools/viewprof.py --only KxWxH --path single|multi`.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402

SHAPES = [(6, 512, 512), (2, 1920, 1080), (8, 960, 540)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", default="")
    ap.add_argument("--path", default="both", choices=("both", "single", "multi"))
    args = ap.parse_args()
    import torch
    pkg = g.load_package()
    S, GM, A = pkg.scenes, pkg.glmath, pkg.abi
    hip = pkg.load_product_library()
    sc = S.sponza_like(lod=1, tex_size=64)
    for k_views, w, h in SHAPES:
        if args.only and args.only != f"{k_views}x{w}x{h}":
            continue
        r = hip.create(w, h)
        handles = sc.upload(r)
        opaque, transparent = sc.render_objects(handles)
        pos, pitch, yaw = S.config3_camera()
        scenes = [S.scene_data_struct(pos, pitch, np.float32(yaw + GM.radians(360.0 * k / k_views)), w, h) for k in range(k_views)]
        lst = r.create_draw_list(opaque, transparent)
        color = torch.zeros((k_views, h, w, 4), dtype=torch.int16, device="cuda")
        depth = torch.zeros((k_views, h, w), dtype=torch.float32, device="cuda")
        cp, dp = color.data_ptr(), depth.data_ptr()
        white = (1.0, 1.0, 1.0, 1.0)

        def single():
            t = 0.0
            for k in range(k_views):
                r.bind_targets(cp + k * w * h * 8, dp + k * w * h * 4)
                r.clear_color(white)
                t += r.draw_list(scenes[k], lst).mesh_draw_time
            r.bind_targets(None, None)
            return t

        def multi():
            return r.draw_list_views(scenes, lst, cp, dp, clear_rgba=white).mesh_draw_time

        paths = {"single": single, "multi": multi}
        if args.path != "both":
            paths = {args.path: paths[args.path]}
        for f in paths.values():  # warm-up
            for _ in range(5):
                f()
        r.sync()
        res = {p: ([], [], [], []) for p in paths}
        for _ in range(args.rounds):
            for p, f in paths.items():
                r.sync()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                host_ms, t0 = 0.0, time.perf_counter()
                for _ in range(args.frames):
                    host_ms += f()
                call_s = time.perf_counter() - t0
                r.sync()
                e1.record()
                e1.synchronize()
                res[p][0].append(e0.elapsed_time(e1) / args.frames * 1e3)
                res[p][1].append(host_ms / args.frames * 1e3)
                res[p][2].append(call_s / args.frames * 1e6)
                fenced = 0.0
                for _ in range(args.frames):
                    fenced += f()
                    r.sync()
                res[p][3].append(fenced / args.frames * 1e3)
        lst.close()
        r.close()
        line = f"{k_views} x {w}x{h}:"
        for p, (fr, ho, ca, fe) in res.items():
            line += (f"  {p}: frame {np.median(fr):7.1f} us, library host {np.median(ho):6.1f} us (fenced {np.median(fe):6.1f}),"
                     f" calls {np.median(ca):6.1f} us")
        if len(res) == 2:
            line += f"  multi/single frame {np.median(res['multi'][0]) / np.median(res['single'][0]):.3f}"
        print(line, flush=True)


if __name__ == "__main__":
    main()
