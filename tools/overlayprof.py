"""Developer tool: what the UI overlay pass (include/svr_overlay.h) costs on the MI355X, at 3840x2160 and 1920x1080:

    stats_window     the list svr_demo --stats-overlay 1 draws: one window, five lines of text
    ui_2k            about 2,000 triangles of text in six windows that cover a tenth of the screen
    ui_20k           about 20,000 triangles of text in four windows that cover half the screen
    fullscreen_quad  two translucent triangles over everything: the read-modify-write floor, 8 bytes per pixel
    blit             the identity svr_copy_to_swapchain of the same extent, the yardstick: the operation an overlay follows

Every figure is device time: two events on the context's stream around a window of --reps calls that starts from a fenced,
idle stream, divided by the calls.  The stages alternate inside every round, round 0 warms up, and the median, lowest and
highest window of the --rounds others are kept, so the run-to-run spread stands beside every figure.  A call includes the
copy of the list to the device in front of the kernels.  Byte model: an overlay reads and writes 4 B per texel of the tiles
with work (the records and the atlas are not counted); the blit reads 8 B and writes 4 B per pixel.

    python tools/overlayprof.py [--reps 20] [--rounds 9] [--out profiles/overlay_cost.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402

INK = (255, 255, 255, 255)
FILLER = "FRAMETIME:16.667MS/DRAWS-1024+TRIANGLES(262144)_UPDATE,0.031%"


def stats_window(builder):
    builder.window(10, 10, 150, 64, "stats")
    for k, line in enumerate(["frametime 16.666668 ms", "draw time 1.250000 ms", "update time 0.031000 ms", "triangles 262144", "draws 1024"]):
        builder.text(14, 26 + 9 * k, line, INK)


def text_windows(builder, boxes, glyphs_each, scale):
    """windows full of text: glyphs_each glyphs in each, lines of as many characters as fit"""
    for n, (x, y, w, h) in enumerate(boxes):
        builder.window(x, y, w, h, f"window {n}")
        per_line = max((w - 8) // (6 * scale), 1)
        left, line = glyphs_each, 0
        while left > 0:
            take = min(per_line, left)
            builder.text(x + 4, y + 14 + line * 8 * scale, (FILLER * (take // len(FILLER) + 1))[:take], INK, scale)
            left, line = left - take, line + 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20, help="calls per timed window")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--sizes", default="3840x2160,1920x1080")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "overlay_cost.json"))
    args = ap.parse_args()
    pkg = g.load_package()
    import torch
    if not torch.cuda.is_available():
        sys.exit("overlayprof: no GPU; these are device times and there is no fallback")
    A = pkg.abi
    lib = pkg.load_product_library()
    font = A.overlay_font(lib)
    atlas = torch.from_numpy(font[0].copy()).cuda()
    white = torch.full((1, 1, 4), 255, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    results = []
    for size in args.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        scale = 2 if w >= 3000 else 1
        lists = {}
        b = pkg.overlay.ListBuilder(font)
        stats_window(b)
        lists["stats_window"] = b.arrays()
        b = pkg.overlay.ListBuilder(font)
        text_windows(b, [((k % 3) * (w // 3) + 20, (k // 3) * (h // 2) + 30, w // 5, h // 12) for k in range(6)], 160, scale)
        lists["ui_2k"] = b.arrays()
        b = pkg.overlay.ListBuilder(font)
        text_windows(b, [((k % 2) * (w // 2), (k // 2) * (h // 2) + (k % 2) * (h // 4), w // 2, h // 4) for k in range(4)], 2490, scale)
        lists["ui_20k"] = b.arrays()
        quad = np.zeros(4, A.OVERLAY_VERTEX_DTYPE)
        for k, (x, y) in enumerate([(0, 0), (w, 0), (w, h), (0, h)]):
            quad[k] = ((x, y), (0.5, 0.5), 0x80ff8040)
        cmd = np.zeros(1, A.OVERLAY_CMD_DTYPE)
        cmd[0] = ((0, 0, w, h), 1, 0, 0, 6)
        lists["fullscreen_quad"] = (quad, np.array([0, 1, 2, 0, 2, 3], np.uint16), cmd)
        textures = [(atlas, 96, 48, A.OVERLAY_TEX_A8), (white, 1, 1, A.OVERLAY_TEX_RGBA8)]

        image = torch.zeros((h, w), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        c = lib.create(w, h)
        c.set_stream(stream.cuda_stream)
        c.clear_color((0.2, 0.4, 0.6, 1.0))
        c.sync()
        stages, info = {}, {}
        for name, (v, i, cm) in lists.items():
            stages[name] = (lambda v=v, i=i, cm=cm: c.draw_overlay(image, w, h, 0, v, i, cm, textures))
            stages[name]()
            st = c.read_overlay_stats()
            info[name] = {"triangles": st.triangles, "kept": st.kept, "tiles": st.tiles, "model_bytes": 8 * 1024 * st.tiles}
        stages["blit"] = (lambda: c.copy_to_swapchain(image.data_ptr(), w, h, 0))
        info["blit"] = {"model_bytes": 12 * w * h}

        def window(call):
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
            for k, call in stages.items():
                t = window(call)
                if rnd:
                    ms[k].append(t)
        out = {"width": w, "height": h, "reps": args.reps, "rounds": args.rounds, "stages": {}}
        for k in stages:
            a = np.array(ms[k])
            med = float(np.median(a))
            out["stages"][k] = dict(info[k], ms=round(med, 4), min_ms=round(float(a.min()), 4), max_ms=round(float(a.max()), 4),
                                    spread_pct=round(100.0 * float(a.max() - a.min()) / med, 1),
                                    tb_per_s=round(info[k]["model_bytes"] / (med * 1e-3) / 1e12, 3))
        st = out["stages"]
        out["vs_blit"] = {k: round(st[k]["ms"] / st["blit"]["ms"], 3) for k in lists}
        print(json.dumps(out), flush=True)
        results.append(out)
        c.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/overlayprof.py", "device": torch.cuda.get_device_name(0), "sizes": results}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
