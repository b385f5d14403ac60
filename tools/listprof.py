"""Developer tool: library host time per pass of svr_draw_geometry against svr_draw_list (include/svr_draw_list.h),
with an idle GPU (every pass is fenced), on configs[2], configs[3], a band of an eight-way split of configs[3] and
configs[4].  Host time = SvrStats.mesh_draw_time, the time spent inside the call.

    python tools/listprof.py [--frames 300] [--only NAME:PATH]

Chip time of the stage-1 chain (prologue, flatten kernels, setup, bin count / scan / fill): run one NAME:PATH at a time
under `rocprofv3 --kernel-trace --stats -- python tools/listprof.py --only NAME:PATH --frames 100` and add the
kernel_stats of every kernel but tile_kernel and report_kernel, divided by the passes (--frames + 5 warm-up).
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402

# name -> (width, height, scissor rows or None, instanced)
CONFIGS = {
    "config2": (1920, 1080, None, False),
    "config3": (3840, 2160, None, False),
    "config3_band8": (3840, 2160, (0, 270), False),
    "config4": (7680, 4320, None, True),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--only", default="", help="NAME:PATH, PATH = geometry | list")
    args = ap.parse_args()
    pkg = g.load_package()
    S = pkg.scenes
    hip = pkg.load_product_library()
    sc = S.sponza_like(lod=1, tex_size=64)
    only = tuple(args.only.split(":")) if args.only else None
    for name, (w, h, rows, instanced) in CONFIGS.items():
        if only and only[0] != name:
            continue
        r = hip.create(w, h)
        handles = sc.upload(r)
        opaque, transparent = sc.render_objects(handles, instance_transforms=S.config5_instances() if instanced else None)
        cam = S.config5_camera() if instanced else S.config3_camera()
        scene = S.scene_data_struct(*cam, w, h)
        if rows:
            r.set_scissor(0, rows[0], w, rows[1])
        lst = r.create_draw_list(opaque, transparent)
        res = {}
        for path in ("geometry", "list"):
            if only and only[1] != path:
                continue
            draw = (lambda: r.draw_geometry(scene, opaque, transparent)) if path == "geometry" else (lambda: r.draw_list(scene, lst))
            lib_us, call_us = [], []
            for k in range(args.frames + 5):
                r.clear_color((1, 1, 1, 1))
                t0 = time.perf_counter()
                st = draw()
                t1 = time.perf_counter()
                r.sync()
                if k >= 5:
                    lib_us.append(st.mesh_draw_time * 1e3)
                    call_us.append((t1 - t0) * 1e6)
            res[path] = (np.median(lib_us), np.median(call_us))
        lst.close()
        r.close()
        n = len(opaque) + len(transparent)
        print(f"{name:14s} {n:5d} objects  " + "  ".join(
            f"{p}: library {lib:6.1f} us, call {call:6.1f} us" for p, (lib, call) in res.items()), flush=True)


if __name__ == "__main__":
    main()
