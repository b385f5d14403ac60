"""Developer tool: what the ID target (include/svr_ids.h) costs per frame, bench.py's workload (configs[3], 3840x2160,
lod 1, 1024^2 textures) by default.  Frames are pipelined as bench.py runs them (no fence between them); blocks of
--frames with IDs off and on alternate, and the median ms per frame of each side is printed as one JSON line.

    python tools/idcost.py [--frames 200] [--blocks 5] [--width 3840 --height 2160]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--tex-size", type=int, default=1024)
    args = ap.parse_args()
    pkg = g.load_package()
    S = pkg.scenes
    hip = pkg.load_product_library()
    sc = S.sponza_like(lod=1, tex_size=args.tex_size)
    r = hip.create(args.width, args.height)
    opaque, transparent = sc.render_objects(sc.upload(r))
    scene = S.scene_data_struct(*S.config3_camera(), args.width, args.height)
    r.set_option(pkg.abi.OPT_COUNT_FRAGMENTS, 0)

    def block(ids):
        r.enable_ids(ids)
        for _ in range(5):
            r.draw_geometry(scene, opaque, transparent)
        r.sync()
        t0 = time.perf_counter()
        for _ in range(args.frames):
            r.clear_color((1, 1, 1, 1))
            r.draw_geometry(scene, opaque, transparent)
        r.sync()
        return (time.perf_counter() - t0) * 1e3 / args.frames

    t_end = time.perf_counter() + 1.0  # settle the clocks
    while time.perf_counter() < t_end:
        r.draw_geometry(scene, opaque, transparent)
    r.sync()
    off, on = [], []
    for _ in range(args.blocks):
        off.append(block(False))
        on.append(block(True))
    r.close()
    m_off, m_on = float(np.median(off)), float(np.median(on))
    print(json.dumps({"width": args.width, "height": args.height, "ms_per_frame_ids_off": round(m_off, 4),
                      "ms_per_frame_ids_on": round(m_on, 4), "cost_ms": round(m_on - m_off, 4),
                      "cost_pct": round(100.0 * (m_on - m_off) / m_off, 2), "blocks_off": [round(x, 4) for x in off],
                      "blocks_on": [round(x, 4) for x in on]}))


if __name__ == "__main__":
    main()
