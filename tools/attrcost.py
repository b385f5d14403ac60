"""Developer tool: what the attribute targets (include/svr_attributes.h) cost the tile kernel, on bench.py's workload
(configs[3], lod 1, 1024^2 textures) at 3840x2160 and 1920x1080.  For every attribute mask (none, each single plane, all
four) blocks of --frames pipelined frames are timed with SVR_OPT_KERNEL_TIMING = 1 (SvrStats.tile_ms: the tile kernel
alone, by events on its own dispatch); the masks alternate inside every round, all in one process.  Printed per mask:
the median tile_ms over the rounds, the added time against mask 0, and the floor the added bytes imply (the planes'
bytes over --hbm-write-tbs, the achievable HBM write rate).  One JSON line per size.

    python tools/attrcost.py [--frames 40] [--rounds 9] [--libs build_ab/libsvr_hip_x.so ...]

--libs: further builds of the library measured beside the product in the same rounds (store-shape variants of
tools/build_variant.sh; a build without attribute targets is measured at mask 0 only).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402

MASKS = (0, 1, 2, 4, 8, 15)
TEXEL_BYTES = {1: 16, 2: 8, 4: 16, 8: 16}


def plane_bytes(mask, w, h):
    return sum(b for bit, b in TEXEL_BYTES.items() if mask & bit) * w * h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--sizes", default="3840x2160,1920x1080")
    ap.add_argument("--hbm-write-tbs", type=float, default=6.0, help="achievable HBM write rate, TB/s")
    ap.add_argument("--libs", nargs="*", default=[])
    args = ap.parse_args()
    pkg = g.load_package()
    import torch  # noqa: F401  (one HIP runtime per process: torch's is loaded first)
    S, A = pkg.scenes, pkg.abi
    sc = S.sponza_like(lod=1, tex_size=1024)
    libs = [("product", pkg.load_product_library())] + [(os.path.basename(p), A.SvrLib(os.path.abspath(p))) for p in args.libs]
    for size in args.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        scene = S.scene_data_struct(*S.config3_camera(), w, h)
        ctx = []
        for name, lib in libs:
            r = lib.create(w, h)
            opaque, transparent = sc.render_objects(sc.upload(r))
            r.set_option(A.OPT_COUNT_FRAGMENTS, 0)
            ctx.append((name, r, opaque, transparent, MASKS if lib.has_attributes else (0,)))

        def block(r, opaque, transparent, mask, frames):
            if r.lib.has_attributes:
                r.enable_attributes(mask)
            for _ in range(3):
                r.draw_geometry(scene, opaque, transparent)
            r.sync()
            r.set_option(A.OPT_KERNEL_TIMING, 1)  # (resets the running mean)
            for _ in range(frames):
                r.clear_color((1, 1, 1, 1))
                r.draw_geometry(scene, opaque, transparent)
            r.sync()
            ms = r.get_stats().tile_ms
            r.set_option(A.OPT_KERNEL_TIMING, 0)
            return ms

        res = {(name, m): [] for name, _r, _o, _t, masks in ctx for m in masks}
        for rnd in range(args.rounds + 1):  # round 0 warms up
            for name, r, opaque, transparent, masks in ctx:
                for m in masks:
                    ms = block(r, opaque, transparent, m, args.frames)
                    if rnd:
                        res[(name, m)].append(ms)
        out = {"width": w, "height": h, "frames": args.frames, "rounds": args.rounds, "hbm_write_tbs": args.hbm_write_tbs, "libs": {}}
        for name, _r, _o, _t, masks in ctx:
            base = float(np.median(res[(name, 0)]))
            d = {}
            for m in masks:
                a = np.array(res[(name, m)])
                floor_ms = plane_bytes(m, w, h) / (args.hbm_write_tbs * 1e12) * 1e3
                d[str(m)] = {"tile_ms": round(float(np.median(a)), 4), "min": round(float(a.min()), 4), "max": round(float(a.max()), 4),
                             "added_ms": round(float(np.median(a)) - base, 4), "added_pct": round(100.0 * (float(np.median(a)) - base) / base, 1),
                             "plane_mb": round(plane_bytes(m, w, h) / 1e6, 1), "floor_ms": round(floor_ms, 4)}
            out["libs"][name] = d
        print(json.dumps(out), flush=True)
        for _name, r, *_rest in ctx:
            r.close()


if __name__ == "__main__":
    main()
