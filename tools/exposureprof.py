"""Developer tool: what auto-exposure (include/svr_exposure.h) costs on the MI355X, at 3840x2160 and 1920x1080:

    svr_meter_exposure over three inputs bound as the colour target
        lit       bench.py's workload (configs[3], lod 1, 1024^2 textures): G-buffer pass, lighting pass with 1024 lights
        constant  one value everywhere: every lane of every wave counts into one bin
        noise     log2-uniform values over 2^-12 .. 2^12: the lanes of a wave scatter over some two hundred bins
    svr_post_pass with 0 bloom levels over the lit input, the yardstick: it reads the same bytes and writes them back
    svr_post_pass with 0 and with 5 levels under svr_set_post_auto_exposure, beside the same passes with it off

Every figure is device time: two events on the context's stream around a window of --reps calls that starts from a fenced,
idle stream, divided by the calls.  The stages alternate inside every round, round 0 warms up, and the median, lowest and
highest window of the --rounds others are kept, so the run-to-run spread stands beside every figure.  The meter's cost
depends on the values only through the contention on its LDS counters, which is what the three inputs are for.  Byte model:
the meter reads 8 B per pixel of the scissor once (its 2 KB of bins and state are not counted); post with 0 levels reads and
writes 8 B per pixel.

--also PATH[,PATH...] times the same stages on other builds of the library in the same rounds, interleaved with this one's
(the parent's build for the post pass's A/B; a -DSVR_AB_EXPOSURE_NO_PEEL build for the LDS scheme's): a build without
auto-exposure runs the post stages only.

    python tools/exposureprof.py [--reps 20] [--rounds 9] [--also build_ab/libsvr_hip_parent.so] [--out profiles/exposure_cost.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import __graft_entry__ as g  # noqa: E402
from postprof import post_bytes, surface_lights  # noqa: E402

TEXEL = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20, help="calls per timed window")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--sizes", default="3840x2160,1920x1080")
    ap.add_argument("--also", default="", help="other builds of libsvr_hip.so to time in the same rounds, comma separated")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exposure_cost.json"))
    args = ap.parse_args()
    pkg = g.load_package()
    import torch
    if not torch.cuda.is_available():
        sys.exit("exposureprof: no GPU; these are device times and there is no fallback")
    S, A = pkg.scenes, pkg.abi
    libs = [("this", pkg.load_product_library())] + [(os.path.basename(p), A.SvrLib(os.path.abspath(p))) for p in args.also.split(",") if p]
    sc = S.sponza_like(lod=1, tex_size=1024)
    empty = np.zeros(0, A.RENDER_OBJECT_DTYPE)
    stream = torch.cuda.Stream()
    results = []
    for size in args.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        scene = S.scene_data_struct(*S.config3_camera(), w, h)
        # the lit frame, rendered once by this build
        r = libs[0][1].create(w, h)
        opaque, _transparent = sc.render_objects(sc.upload(r))
        r.set_option(A.OPT_COUNT_FRAGMENTS, 0)
        r.enable_attributes(A.ATTR_NORMAL | A.ATTR_ALBEDO)
        r.clear_color((1, 1, 1, 1))
        r.draw_geometry(scene, opaque, empty)
        m = np.asarray(scene.viewproj, dtype=np.float64).reshape(4, 4).T
        inv_vp = np.ascontiguousarray(np.linalg.inv(m).T.reshape(16), dtype=np.float32)
        lights = surface_lights(1024, r.read_depth(), inv_vp, A.POINT_LIGHT_DTYPE, seed=1)
        r.light_pass(inv_vp, np.array(scene.ambient_color, np.float32), np.array(scene.sunlight_direction, np.float32),
                     np.array(scene.sunlight_color, np.float32), lights=lights)
        lit = r.read_color()
        r.close()
        rng = np.random.default_rng(5)
        with np.errstate(over="ignore"):
            noise = (2.0 ** rng.uniform(-12, 12, (h, w, 4))).astype(np.float32).astype(np.float16).view(np.uint16)
        constant = np.full((h, w, 4), np.float16(0.37).view(np.uint16), np.uint16)
        planes = {k: torch.from_numpy(np.ascontiguousarray(v).view(np.int32).reshape(h, w, 2).copy()).cuda()
                  for k, v in (("lit", lit), ("constant", constant), ("noise", noise))}
        posted = planes["lit"].clone()  # the post pass works in place: it gets a plane of its own (its cost does not depend on the values)
        depth = torch.zeros((h, w), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()

        stages = {}  # name -> (context, call, bytes)
        for name, lib in libs:
            tag = "" if name == "this" else "@" + name
            if getattr(lib, "has_exposure", False):
                for plane in planes:
                    c = lib.create(w, h)
                    c.set_stream(stream.cuda_stream)
                    c.bind_targets(planes[plane].data_ptr(), depth.data_ptr())
                    stages[f"meter_{plane}{tag}"] = (c, (lambda c=c: c.meter_exposure(0.18, 0.05, 0.95, 2.0 ** -10, 2.0 ** 10, 0.25)), TEXEL * w * h)
            plain = lib.create(w, h)
            plain.set_stream(stream.cuda_stream)
            plain.bind_targets(posted.data_ptr(), depth.data_ptr())
            for levels in (0, 5):
                nbytes = sum(post_bytes(w, h, levels).values())
                stages[f"post_{levels}{tag}"] = (plain, (lambda c=plain, n=levels: c.post_pass(1.0, 1.0, 0.5, n, A.TONEMAP_ACES)), nbytes)
                if getattr(lib, "has_exposure", False):
                    auto = lib.create(w, h)
                    auto.set_stream(stream.cuda_stream)
                    auto.bind_targets(posted.data_ptr(), depth.data_ptr())
                    auto.set_post_auto_exposure(True)
                    stages[f"post_{levels}_auto{tag}"] = (auto, (lambda c=auto, n=levels: c.post_pass(1.0, 1.0, 0.5, n, A.TONEMAP_ACES)), nbytes)

        def window(c, call):
            c.sync()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(stream)
            for _ in range(args.reps):
                call()
            t1.record(stream)
            t1.synchronize()
            c.sync()
            return t0.elapsed_time(t1) / args.reps

        ms = {k: [] for k in stages}
        for rnd in range(args.rounds + 1):  # round 0 warms up
            for k, (c, call, _b) in stages.items():
                t = window(c, call)
                if rnd:
                    ms[k].append(t)
        out = {"width": w, "height": h, "reps": args.reps, "rounds": args.rounds, "stages": {}}
        for k, (_c, _call, nbytes) in stages.items():
            a = np.array(ms[k])
            med = float(np.median(a))
            out["stages"][k] = {"ms": round(med, 4), "min_ms": round(float(a.min()), 4), "max_ms": round(float(a.max()), 4),
                                "spread_pct": round(100.0 * float(a.max() - a.min()) / med, 1), "model_mb": round(nbytes / 1e6, 2),
                                "tb_per_s": round(nbytes / (med * 1e-3) / 1e12, 3)}
        st = out["stages"]
        out["meter_vs_post_0"] = {p: round(st[f"meter_{p}"]["ms"] / st["post_0"]["ms"], 3) for p in planes}
        print(json.dumps(out), flush=True)
        results.append(out)
        for c, _call, _b in stages.values():
            c.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/exposureprof.py", "device": torch.cuda.get_device_name(0), "also": args.also, "sizes": results}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
