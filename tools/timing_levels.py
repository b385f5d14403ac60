"""Developer tool: SvrStats.tile_ms of the same frames at SVR_OPT_KERNEL_TIMING level 1 (the tile kernel's own clock
stamps) and level 2 (event records around every stage), twelve-pass means, three repetitions per size.

    python tools/timing_levels.py [--sizes 96x54,128x72,3840x2160] [--lib build_ab/libsvr_hip_x.so]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="96x54,128x72,3840x2160")
    ap.add_argument("--lib", default="", help="another build of libsvr_hip.so instead of the product's")
    args = ap.parse_args()
    pkg = g.load_package()
    S, A = pkg.scenes, pkg.abi
    hip = A.SvrLib(os.path.abspath(args.lib)) if args.lib else pkg.load_product_library()
    for size in args.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        sc = S.sponza_like(lod=8 if w < 1000 else 1, tex_size=64)
        r = hip.create(w, h)
        opaque, transparent = sc.render_objects(sc.upload(r))
        scene = S.scene_data_struct(*S.config3_camera(), w, h)

        def frames(n):
            for _ in range(n):
                r.clear_color((1, 1, 1, 1))
                r.draw_geometry(scene, opaque, transparent)
            r.sync()

        frames(4)
        for rep in range(3):
            res = {}
            for level in (1, 2):
                r.set_option(A.OPT_KERNEL_TIMING, level)
                frames(12)
                st = r.get_stats()
                res[level] = (st.tile_ms, st.timed_passes)
            print(f"{w}x{h} rep {rep}: level1 tile_ms {res[1][0]:.5f} ({res[1][1]} passes)  level2 tile_ms {res[2][0]:.5f} "
                  f"({res[2][1]} passes)  diff {1e3 * (res[2][0] - res[1][0]):.2f} us", flush=True)
        r.set_option(A.OPT_KERNEL_TIMING, 0)
        r.close()


if __name__ == "__main__":
    main()
