"""A small list builder for the UI overlay pass (include/svr_overlay.h) on top of the built-in font: rectangles, text and
windows, emitted as the vertices, 16-bit indices and commands Renderer.draw_overlay takes.  host/svr_overlay_text.h is
the same builder in C++: both make the same arrays, bit for bit, from the same calls.

    b = overlay.ListBuilder(abi.overlay_font(lib))
    b.window(16, 16, 200, 80, "stats")
    b.text(22, 34, "frametime 1.25 ms", (255, 255, 255, 255))
    vertices, indices, cmds = b.arrays()
    renderer.draw_overlay(image, w, h, fmt, vertices, indices, cmds, [(atlas_on_device, 96, 48, abi.OVERLAY_TEX_A8)])
"""
import numpy as np

from . import abi

f32 = np.float32
WINDOW_BODY, WINDOW_BAR, WINDOW_TITLE = (20, 20, 24, 200), (48, 72, 120, 255), (255, 255, 255, 255)
WINDOW_BAR_HEIGHT = 12
NO_CLIP = (0.0, 0.0, 16384.0, 16384.0)  # of what is drawn outside any window


def pack(rgba):
    r, g, b, a = (int(v) & 0xff for v in rgba)
    return r | (g << 8) | (b << 16) | (a << 24)


class ListBuilder:
    """font: abi.overlay_font()'s tuple; texture: the atlas's index in the texture table the list is drawn with"""

    def __init__(self, font, texture=0):
        atlas, self.cell_w, self.cell_h, self.first, self.n_chars = font
        self.atlas_h, self.atlas_w = atlas.shape
        self.texture = texture
        self.v, self.i, self.c = [], [], []  # vertices (x, y, u, v, col), indices, commands [clip, vtx_offset, idx_offset, elem_count]
        self.white = (f32(abi.OVERLAY_FONT_WHITE_X + 0.5) / f32(self.atlas_w), f32(abi.OVERLAY_FONT_WHITE_Y + 0.5) / f32(self.atlas_h))

    def _command(self, clip):
        self.c.append([tuple(float(x) for x in clip), len(self.v), len(self.i), 0])

    def _quad(self, x0, y0, x1, y1, u0, v0, u1, v1, col):
        if not self.c:
            self._command(NO_CLIP)
        cmd = self.c[-1]
        base = len(self.v) - cmd[1]
        if base + 4 > 65536:  # 16-bit indices: go on in a new command with the same clip rectangle
            self._command(cmd[0])
            cmd, base = self.c[-1], 0
        self.v += [(x0, y0, u0, v0, col), (x1, y0, u1, v0, col), (x1, y1, u1, v1, col), (x0, y1, u0, v1, col)]
        self.i += [base, base + 1, base + 2, base, base + 2, base + 3]
        cmd[3] += 6

    def rect(self, x, y, w, h, rgba):
        u, v = self.white
        self._quad(f32(x), f32(y), f32(x) + f32(w), f32(y) + f32(h), u, v, u, v, pack(rgba))

    def text(self, x, y, string, rgba, scale=1):
        col, s = pack(rgba), f32(scale)
        gw, gh = f32(self.cell_w) * s, f32(self.cell_h) * s
        px, py = f32(x), f32(y)
        for ch in string:
            if ch == "\n":
                px, py = f32(x), py + gh
                continue
            cell = ord(ch) - self.first
            if not 0 <= cell < self.n_chars:
                cell = self.n_chars  # the filled cell
            if ch != " ":
                cx, cy = cell % 16, cell // 16
                u0, u1 = f32(cx * self.cell_w) / f32(self.atlas_w), f32((cx + 1) * self.cell_w) / f32(self.atlas_w)
                v0, v1 = f32(cy * self.cell_h) / f32(self.atlas_h), f32((cy + 1) * self.cell_h) / f32(self.atlas_h)
                self._quad(px, py, px + gw, py + gh, u0, v0, u1, v1, col)
            px = px + gw

    def window(self, x, y, w, h, title):
        """a new command clipped to the window: its body, a title bar and the title; what follows is drawn inside it"""
        self._command((f32(x), f32(y), f32(x) + f32(w), f32(y) + f32(h)))
        self.rect(x, y, w, h, WINDOW_BODY)
        self.rect(x, y, w, WINDOW_BAR_HEIGHT, WINDOW_BAR)
        self.text(f32(x) + f32(3), f32(y) + f32(2), title, WINDOW_TITLE)

    def arrays(self):
        """-> (vertices OVERLAY_VERTEX_DTYPE, indices uint16, cmds OVERLAY_CMD_DTYPE)"""
        vertices = np.zeros(len(self.v), abi.OVERLAY_VERTEX_DTYPE)
        for k, (x, y, u, v, col) in enumerate(self.v):
            vertices[k] = ((x, y), (u, v), col)
        cmds = np.zeros(len(self.c), abi.OVERLAY_CMD_DTYPE)
        for k, (clip, vtx, idx, n) in enumerate(self.c):
            cmds[k] = (clip, self.texture, vtx, idx, n)
        return vertices, np.asarray(self.i, dtype=np.uint16), cmds
