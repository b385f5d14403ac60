"""Developer tool: count phase A's column walk on the CPU (phase A; numpy only, no GPU, no library).

    python tools/walk_sim.py --width 3840 --height 2160

The frame is bench.py's: scenes.sponza_like() seen from config3_camera(), opaque surfaces only.  Triangles are projected in
float64 (contract C1-C4 without the fp32 roundings: clip volume, near/far planes clipped, snap to 1/256 px, exact integer edge
functions with the top-left rule) and their boxes clamped to 32 x 32 tiles.  Per tile the triangles are taken 64 to a batch in
scene order; a batch's (triangle, column) pairs are cut into 2 / 4 row bands at <= 128 / <= 64 columns and walked as chunks of
64 work items, one lane an item, a wave stepping until its longest lane is done (k_tile.hip scan_columns).  Printed: the walk
as it was (every row of the item's box), the walk over the covered span only (csrc/svr_span.h), and two figures for what this
opens: items without a covered row dropped and the rest regrouped 64 at a time per batch, and spans cut
into pieces of at most 4 / 8 / 16 rows before regrouping.

Not modelled: the draw order of the host's sort (batches hold other triangles of the same tile), the guard band's clipper (a
piece has its own box), split tiles' quarters and the hierarchical depth test (neither runs in the 4K frame), transparent
surfaces (walked by the ordered scan).  tests/test_column_span.py holds the covered-sample count to within 2 % of the
instrumented frame's count at 4K and at 1080p.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402

TILE, BATCH = 32, 64


def _clip_poly(poly, dist):
    """Sutherland-Hodgman against one plane: poly is a list of clip-space points, dist(p) >= 0 is inside."""
    out = []
    for i, a in enumerate(poly):
        b = poly[(i + 1) % len(poly)]
        da, db = dist(a), dist(b)
        if da >= 0:
            out.append(a)
        if (da >= 0) != (db >= 0):
            p, q, dp, dq = (a, b, da, db) if da >= 0 else (b, a, db, da)  # always from the inside vertex
            out.append(p + (dp / (dp - dq)) * (q - p))
    return out


def screen_triangles(pkg, width, height):
    """Opaque triangles of the frame in scene order as snapped integer vertices [n, 3, 2] (1/256 px)."""
    S, A, G = pkg.scenes, pkg.abi, pkg.glmath
    sc = S.sponza_like(lod=1, tex_size=64)  # (geometry does not depend on the texture size)
    pos, pitch, yaw = S.config3_camera()
    viewproj = np.asarray(G.scene_data(G.camera_view(pos, pitch, yaw), width, height)[2], dtype=np.float64)  # [col][row]
    out = []
    for mesh_idx, world in sc.nodes:
        mesh = sc.meshes[mesh_idx]
        p = np.concatenate([mesh.vertices["position"].astype(np.float64), np.ones((mesh.vertices.size, 1))], axis=1)
        clip = (p @ np.asarray(world, dtype=np.float64)) @ viewproj  # row vectors: [col][row] matrices apply from the right
        for s in mesh.surfaces:
            if sc.materials[s.material]["pass_type"] == A.PASS_TRANSPARENT:
                continue
            idx = mesh.indices[s.start_index:s.start_index + s.count].reshape(-1, 3)
            t = clip[idx]  # [n, 3, 4]
            x, y, z, w = t[..., 0], t[..., 1], t[..., 2], t[..., 3]
            reject = ((x < -w).all(1) | (x > w).all(1) | (y < -w).all(1) | (y > w).all(1) | (z < 0).all(1) | (z > w).all(1))
            cut = ~reject & ((z < 0).any(1) | (z > w).any(1))
            keep = t[~reject & ~cut]
            pieces = []
            for tri in t[cut]:  # the few triangles through the near (or far) plane
                poly = _clip_poly(list(tri), lambda q: q[3] - q[2])
                poly = _clip_poly(poly, lambda q: q[2]) if len(poly) >= 3 else []
                for k in range(1, len(poly) - 1):
                    pieces.append(np.stack([poly[0], poly[k], poly[k + 1]]))
            if pieces:
                keep = np.concatenate([keep, np.stack(pieces)])
            if not len(keep):
                continue
            rw = 1.0 / keep[..., 3]
            xs = keep[..., 0] * rw * (width / 2) + width / 2
            ys = keep[..., 1] * rw * (height / 2) + height / 2
            out.append(np.stack([np.rint(xs * 256.0), np.rint(ys * 256.0)], axis=-1).astype(np.int64))
    return np.concatenate(out)


def setup(v, width, height):
    """Per triangle: pixel box clamped to the target and the three biased edge functions e(px, py) = A px + B py + C."""
    X, Y = v[..., 0], v[..., 1]
    area2 = (X[:, 1] - X[:, 0]) * (Y[:, 2] - Y[:, 0]) - (X[:, 2] - X[:, 0]) * (Y[:, 1] - Y[:, 0])
    v = v[area2 != 0]
    area2 = area2[area2 != 0]
    flip = area2 < 0
    v[flip] = v[flip][:, [0, 2, 1]]
    X, Y = v[..., 0], v[..., 1]
    minx = np.maximum(-((-(X.min(1) - 128)) // 256), 0)  # pixel centres at 256 p + 128: ceil / floor
    maxx = np.minimum((X.max(1) - 128) // 256, width - 1)
    miny = np.maximum(-((-(Y.min(1) - 128)) // 256), 0)
    maxy = np.minimum((Y.max(1) - 128) // 256, height - 1)
    ok = (minx <= maxx) & (miny <= maxy)
    Acoef, Bcoef, Ccoef = [], [], []
    for i in range(3):  # edge i runs from vertex i + 1 to i + 2: e(P) = dx (P.y - Ya) - dy (P.x - Xa)
        a, b = (i + 1) % 3, (i + 2) % 3
        dx, dy = X[:, b] - X[:, a], Y[:, b] - Y[:, a]
        bias = np.where((dy < 0) | ((dy == 0) & (dx > 0)), 0, -1)
        Acoef.append(-dy * 256)
        Bcoef.append(dx * 256)
        Ccoef.append(dx * (128 - Y[:, a]) - dy * (128 - X[:, a]) + bias)
    e = np.stack([np.stack(Acoef, 1), np.stack(Bcoef, 1), np.stack(Ccoef, 1)], 1)  # [n, (A B C), edge]
    return minx[ok], maxx[ok], miny[ok], maxy[ok], e[ok]


def _segments(key):
    """Start offsets of the runs of equal values in a sorted key."""
    return np.flatnonzero(np.concatenate([[True], key[1:] != key[:-1]]))


def _wave_steps(group, steps):
    """Items in walk order with their batch (group) and step count: chunks of 64 per group, the longest lane sets the
    chunk's steps.  -> (chunks, wave steps)"""
    if not len(group):
        return 0, 0
    starts = _segments(group)
    idx_in_group = np.arange(len(group)) - np.repeat(starts, np.diff(np.concatenate([starts, [len(group)]])))
    chunk = group * (1 << 20) + idx_in_group // 64
    cs = _segments(chunk)
    return len(cs), int(np.maximum.reduceat(steps, cs).sum())


def simulate(width, height, pkg=None):
    pkg = pkg or g.load_package()
    minx, maxx, miny, maxy, e = setup(screen_triangles(pkg, width, height), width, height)
    tiles_x = (width + TILE - 1) // TILE
    # (triangle, tile) pairs in tile-major, scene order
    tx0, tx1, ty0, ty1 = minx // TILE, maxx // TILE, miny // TILE, maxy // TILE
    nx, ny = tx1 - tx0 + 1, ty1 - ty0 + 1
    tri = np.repeat(np.arange(len(minx)), nx * ny)
    first = np.cumsum(nx * ny) - nx * ny
    k = np.arange(len(tri)) - first[tri]
    px, py = tx0[tri] + k % nx[tri], ty0[tri] + k // nx[tri]
    order = np.lexsort((tri, py * tiles_x + px))
    tri, px, py = tri[order], px[order], py[order]
    tile = py * tiles_x + px
    ts = _segments(tile)
    rank = np.arange(len(tile)) - np.repeat(ts, np.diff(np.concatenate([ts, [len(tile)]])))
    group = np.cumsum(np.concatenate([[0], ((tile[1:] != tile[:-1]) | (rank[1:] % BATCH == 0)).astype(np.int64)]))  # batch id
    cx0, cx1 = np.maximum(minx[tri], px * TILE), np.minimum(maxx[tri], px * TILE + TILE - 1)
    cw = cx1 - cx0 + 1
    total = np.bincount(group, weights=cw).astype(np.int64)
    sh = np.where(total <= 64, 2, np.where(total <= 128, 1, 0))[group]  # log2(bands), per pair
    # items: column-major within the pair, bands innermost (item = column index << sh | band)
    n_items = cw << sh
    pair = np.repeat(np.arange(len(tri)), n_items)
    j = np.arange(len(pair)) - (np.cumsum(n_items) - n_items)[pair]
    shp = sh[pair]
    col = cx0[pair] + (j >> shp)
    band = j & ((1 << shp) - 1)
    band_rows = TILE >> shp
    t = tri[pair]
    y0 = np.maximum(miny[t], py[pair] * TILE + band * band_rows)
    y1 = np.minimum(maxy[t], py[pair] * TILE + band * band_rows + band_rows - 1)
    h = np.maximum(y1 - y0 + 1, 0)
    lo, hi = np.zeros(len(pair), dtype=np.int64), h.copy()  # covered rows [lo, hi) of the item's rows, exact integers
    for i in range(3):
        A, B, C = e[t, 0, i], e[t, 1, i], e[t, 2, i]
        f = A * col + B * y0 + C
        Bs = np.where(B == 0, 1, B)
        lo = np.maximum(lo, np.where(B > 0, -(f // Bs), 0))        # ceil(-f / B)
        hi = np.minimum(hi, np.where(B < 0, f // -Bs + 1, hi))     # floor(f / -B) + 1
        hi = np.where((B == 0) & (f < 0), 0, hi)
    cover = np.maximum(hi - lo, 0)
    gi = group[pair]
    res = {"width": width, "height": height, "triangles": int(len(minx)), "pairs": int(len(tri)), "items": int(len(pair)),
           "items_empty": int((cover == 0).sum()), "lane_steps": int(h.sum()), "covered": int(cover.sum())}
    res["chunks"], res["steps_box"] = _wave_steps(gi, h)
    _, res["steps_span"] = _wave_steps(gi, cover)
    live = cover > 0
    res["chunks_regrouped"], res["steps_regrouped"] = _wave_steps(gi[live], cover[live])
    for cap in (4, 8, 16):
        n_pieces = -(-cover[live] // cap)
        owner = np.repeat(np.arange(int(live.sum())), n_pieces)
        first_piece = (np.cumsum(n_pieces) - n_pieces)[owner]
        rows = np.minimum(cover[live][owner] - (np.arange(len(owner)) - first_piece) * cap, cap)
        res[f"chunks_pieces{cap}"], res[f"steps_pieces{cap}"] = _wave_steps(gi[live][owner], rows)
    return res


def report(r):
    lanes = lambda steps: r["covered"] / float(steps)  # lanes of a wave's 64 that touch a covered row in an average step
    lines = [f"{r['width']}x{r['height']}: {r['triangles']} opaque triangles with a pixel box, {r['pairs']} (triangle, tile) pairs",
             f"covered samples                                      {r['covered']:>10d}",
             f"work items                                           {r['items']:>10d}",
             f"  of which cover no pixel at all                     {r['items_empty']:>10d}  ({100.0 * r['items_empty'] / r['items']:.0f} %)",
             f"lane-steps over box rows                             {r['lane_steps']:>10d}",
             f"  of which covered                                   {r['covered']:>10d}",
             f"chunks of 64 items                                   {r['chunks']:>10d}",
             f"wave-steps, every row of the box (longest box)       {r['steps_box']:>10d}  ({lanes(r['steps_box']):.1f} lanes of 64 covered)",
             f"wave-steps, covered rows only (longest span)         {r['steps_span']:>10d}  ({lanes(r['steps_span']):.1f} lanes)",
             f"wave-steps, empty items dropped, regrouped by batch  {r['steps_regrouped']:>10d}  ({lanes(r['steps_regrouped']):.1f} lanes, {r['chunks_regrouped']} chunks)"]
    for cap in (4, 8, 16):
        s = r[f"steps_pieces{cap}"]
        lines.append(f"  ... spans in pieces of at most {cap:2d} rows              {s:>10d}  ({lanes(s):.1f} lanes, {r[f'chunks_pieces{cap}']} chunks)")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    args = ap.parse_args()
    print(report(simulate(args.width, args.height)))


if __name__ == "__main__":
    main()
