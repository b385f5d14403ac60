"""Developer tool: what the stages of a deferred frame cost on the MI355X, the HDR post pass (include/svr_post.h) among
them, on bench.py's workload (configs[3], lod 1, 1024^2 textures) at 3840x2160 and 1920x1080:

    the G-buffer pass (opaque objects, NORMAL and ALBEDO planes)      svr_draw_geometry
    the lighting pass with 0 and with 1024 point lights               svr_light_pass
    the post pass with 0 and with 5 bloom levels (ACES)               svr_post_pass
    the identity copy to an R8G8B8A8 swapchain image                  svr_copy_to_swapchain

Every figure is device time: two events on the context's stream around a window of --reps calls that starts from a fenced,
idle stream, divided by the calls.  The stages alternate inside every round, round 0 warms up, and the median, lowest and
highest window of the --rounds others are kept, so the run-to-run spread stands beside every figure.  The kernels' cost does
not depend on the values in the targets (no branch of them does), so calling the in-place post pass again and again on its
own output times the same work.  bytes/s come from the byte models below, which count every byte a stage must move once:

    copy      8 B read + 4 B written per pixel
    lighting  44 B per pixel (DESIGN.md §5 "Deferred lighting": depth 4, normal 16, albedo 16, colour 8)
    post      level 0 reads the scissor (8 B per pixel) and writes B_0 (8 B per texel); level i reads B_{i-1} and writes
              B_i; the upsample of level i reads B_i and U_{i+1} and writes U_i; the composite reads the scissor and U_0
              and writes the scissor.  Re-reads of a smaller level's taps are served by the caches and are not counted.
    G-buffer  no model (its traffic depends on the scene): time only

    python tools/postprof.py [--reps 20] [--rounds 9] [--out profiles/post_cost.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402

LIGHT_BYTES_PER_PIXEL = 44
COPY_BYTES_PER_PIXEL = 12
TEXEL = 8  # an RGBA16F texel, and a texel of a level image


def level_extents(w, h, levels):
    out = []
    for _ in range(levels):
        w, h = (w + 1) // 2, (h + 1) // 2
        out.append((w, h))
    return out


def post_bytes(w, h, levels):
    """-> {kernel: bytes} of one post pass over a w x h scissor"""
    ext = level_extents(w, h, levels)
    px = [w * h] + [a * b for a, b in ext]  # px[0]: the scissor; px[i + 1]: level i
    level = sum(TEXEL * (px[i] + px[i + 1]) for i in range(levels))
    up = sum(TEXEL * (2 * px[i + 1] + px[i + 2]) for i in range(levels - 1))
    composite = TEXEL * (2 * px[0] + (px[1] if levels else 0))
    return {"bloom_level_kernel": level, "bloom_up_kernel": up, "post_composite_kernel": composite}


def surface_lights(n, depth, inv_vp, dtype, seed):
    """n seeded point lights on surface points of the frame (positions unprojected in float64), radii log-uniform from
    0.05 to 70 world units: from under one tile's footprint to the whole atrium, as the lighting tests draw them"""
    rng = np.random.default_rng(seed)
    h, w = depth.shape
    ys, xs = np.nonzero(depth > 0)
    pick = rng.integers(0, len(ys), n)
    y, x = ys[pick], xs[pick]
    ndc = np.stack([(x + 0.5) * 2.0 / w - 1.0, (y + 0.5) * 2.0 / h - 1.0, depth[y, x].astype(np.float64), np.ones(n)], axis=1)
    p = ndc @ np.asarray(inv_vp, np.float64).reshape(4, 4)  # column-major [col][row]
    L = np.zeros(n, dtype)
    L["position"] = (p[:, :3] / p[:, 3:4] + rng.normal(0, 0.4, (n, 3))).astype(np.float32)
    L["radius"] = (10.0 ** rng.uniform(np.log10(0.05), np.log10(70.0), n)).astype(np.float32)
    L["color"] = rng.uniform(0.2, 1.0, (n, 3)).astype(np.float32)
    L["intensity"] = rng.uniform(0.5, 4.0, n).astype(np.float32)
    return L


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20, help="calls per timed window")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--sizes", default="3840x2160,1920x1080")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "post_cost.json"))
    args = ap.parse_args()
    pkg = g.load_package()
    import torch
    if not torch.cuda.is_available():
        sys.exit("postprof: no GPU; these are device times and there is no fallback")
    S, A = pkg.scenes, pkg.abi
    lib = pkg.load_product_library()
    sc = S.sponza_like(lod=1, tex_size=1024)
    empty = np.zeros(0, A.RENDER_OBJECT_DTYPE)
    stream = torch.cuda.Stream()
    results = []
    for size in args.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        scene = S.scene_data_struct(*S.config3_camera(), w, h)
        r = lib.create(w, h)
        r.set_stream(stream.cuda_stream)
        opaque, _transparent = sc.render_objects(sc.upload(r))
        r.set_option(A.OPT_COUNT_FRAGMENTS, 0)
        r.enable_attributes(A.ATTR_NORMAL | A.ATTR_ALBEDO)
        r.clear_color((1, 1, 1, 1))
        r.draw_geometry(scene, opaque, empty)
        m = np.asarray(scene.viewproj, dtype=np.float64).reshape(4, 4).T
        inv_vp = np.ascontiguousarray(np.linalg.inv(m).T.reshape(16), dtype=np.float32)
        lights = surface_lights(1024, r.read_depth(), inv_vp, A.POINT_LIGHT_DTYPE, seed=1)
        sun = (np.array(scene.ambient_color, np.float32), np.array(scene.sunlight_direction, np.float32), np.array(scene.sunlight_color, np.float32))
        swap = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

        def gbuffer():
            r.clear_color((1, 1, 1, 1))
            r.draw_geometry(scene, opaque, empty)

        stages = {
            "gbuffer": (gbuffer, None),
            "light_0": (lambda: r.light_pass(inv_vp, *sun), LIGHT_BYTES_PER_PIXEL * w * h),
            "light_1024": (lambda: r.light_pass(inv_vp, *sun, lights=lights), LIGHT_BYTES_PER_PIXEL * w * h),
            "post_0": (lambda: r.post_pass(1.0, 1.0, 0.5, 0, A.TONEMAP_ACES), sum(post_bytes(w, h, 0).values())),
            "post_5": (lambda: r.post_pass(1.0, 1.0, 0.5, 5, A.TONEMAP_ACES), sum(post_bytes(w, h, 5).values())),
            "copy_identity": (lambda: r.copy_to_swapchain(swap.data_ptr(), w, h, 0), COPY_BYTES_PER_PIXEL * w * h),
        }

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
            for k, (call, _b) in stages.items():
                t = window(call)
                if rnd:
                    ms[k].append(t)
        out = {"width": w, "height": h, "reps": args.reps, "rounds": args.rounds, "stages": {},
               "post_5_bytes_by_kernel": post_bytes(w, h, 5), "post_0_bytes_by_kernel": post_bytes(w, h, 0)}
        for k, (_call, nbytes) in stages.items():
            a = np.array(ms[k])
            med = float(np.median(a))
            d = {"ms": round(med, 4), "min_ms": round(float(a.min()), 4), "max_ms": round(float(a.max()), 4),
                 "spread_pct": round(100.0 * float(a.max() - a.min()) / med, 1)}
            if nbytes is not None:
                d["model_mb"] = round(nbytes / 1e6, 2)
                d["tb_per_s"] = round(nbytes / (med * 1e-3) / 1e12, 3)
            out["stages"][k] = d
        out["post_5_vs_copy_rate"] = round(out["stages"]["post_5"]["tb_per_s"] / out["stages"]["copy_identity"]["tb_per_s"], 3)
        out["post_0_vs_copy_rate"] = round(out["stages"]["post_0"]["tb_per_s"] / out["stages"]["copy_identity"]["tb_per_s"], 3)
        print(json.dumps(out), flush=True)
        results.append(out)
        r.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/postprof.py", "device": torch.cuda.get_device_name(0), "sizes": results}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
