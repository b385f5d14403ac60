"""Pins tests/native/light_ref.cpp, the reference of the lighting tests, to the CPU oracle: with no point lights and no
shadow map the lighting contract is C10 evaluated again from the stored normal and albedo, so fed the oracle's own trace
of every pixel it must reproduce the oracle's colour target bit for bit: under the scene's lighting, and under another
sun and ambient against the oracle's frame drawn with those.  CPU only."""
import numpy as np

import __graft_entry__ as g
import lighting_ref as LR
import scenarios as SC
import svr_testlib as T

pkg = g.load_package()
A = pkg.abi
f32 = np.float32

SCENARIO = "floor_trilinear"  # 96 x 64 = 6144 pixels, opaque only: a textured ground plane below the horizon, background above
MIN_WINNERS = 1024
OTHER_LIGHTING = ((0.05, 0.2, 0.15, 1.0), (0.6, 0.3, -0.7, 0.0), (1.0, 0.9, 0.8, 0.7))  # ambient, sun direction, sun colour


def render(lib, mp, lighting=None, trace=False):
    """the scenario through `lib`, opaque objects only, with its lighting replaced or not; trace: also one traced pass per
    pixel -> the frame, plus "scene", "normal", "albedo" (zero texels where no opaque fragment won)"""
    orig_draw, extra = A.Renderer.draw_geometry, {}

    def draw(self, scene, opaque, transparent=None):
        assert transparent is None or len(transparent) == 0
        if lighting is not None:
            scene.ambient_color, scene.sunlight_direction, scene.sunlight_color = (A._f4(v) for v in lighting)
        extra["scene"] = scene
        if trace:
            w, h = self.width, self.height
            normal, albedo = np.zeros((h, w, 4), f32), np.zeros((h, w, 4), f32)
            empty = np.zeros(0, A.RENDER_OBJECT_DTYPE)
            for y in range(h):
                for x in range(w):
                    self.trace_pixel(x, y)
                    orig_draw(self, scene, opaque, empty)
                    t = self.read_trace()
                    if t[0] != 0.0:
                        normal[y, x] = (t[15], t[16], t[17], t[21])
                        albedo[y, x] = (t[18], t[19], t[20], 1.0)
            self.trace_pixel(-1, -1)
            extra["normal"], extra["albedo"] = normal, albedo
        return orig_draw(self, scene, opaque, transparent)

    with mp.context() as m:
        m.setattr(A.Renderer, "draw_geometry", draw)
        out = SC.SCENARIOS[SCENARIO](lib)
    out.update(extra)
    return out


def test_light_ref_reproduces_the_oracle(oracle, monkeypatch):
    base = render(oracle, monkeypatch, trace=True)
    h, w = base["depth"].shape
    assert w * h <= 8192
    inv_vp = LR.inv_viewproj(base["scene"].viewproj)
    for what, lighting in (("the scene's lighting", None), ("another sun and ambient", OTHER_LIGHTING)):
        frame = base if lighting is None else render(oracle, monkeypatch, lighting=lighting)
        ambient, sun_dir, sun_color = LR.lighting_of(frame["scene"])
        if lighting is not None:
            assert np.array_equal(ambient, np.array(lighting[0], f32)) and np.array_equal(sun_dir, np.array(lighting[1], f32))
            assert not np.array_equal(frame["color"], base["color"]), "the other lighting must change the frame"
            T.assert_images_identical(frame["depth"], base["depth"], "depth under another lighting")
        ref = LR.run_ref(base["depth"], base["normal"], base["albedo"], inv_vp, ambient, sun_dir, sun_color)
        win = ref["winner"]
        assert np.array_equal(win, base["albedo"][..., 3] == 1.0)
        assert int(win.sum()) >= MIN_WINNERS, f"only {int(win.sum())} pixels have an opaque winner"
        got = LR.store(ref["rgba"], A.COLOR_RGBA16F)
        bad = np.any(got != frame["color"], axis=-1) & win
        assert not bad.any(), f"{what}: {int(bad.sum())} of {int(win.sum())} winner pixels differ from the oracle, first at (y, x) = {np.argwhere(bad)[0].tolist()}"
        print(f"{what}: {int(win.sum())} winner pixels of {w * h} equal the oracle's colour target")
