"""Every scenario through the tile-kernel instances bench.py times.

The scenarios render instrumented (scenarios.Rig sets SVR_OPT_COUNT_FRAGMENTS), and instrumented passes drop nothing:
only the uninstrumented tile_kernel<FMT, false, SPLIT> drops triangles with the hierarchical depth test (the occluder
claim and the 8x8 block minima of scan_columns, the deep-bin filter of tile_body).  Here each scenario runs on the HIP
library uninstrumented with the test automatic, off, forced, and forced without split tiles (the only setting that
launches SPLIT = false), and instrumented with the test forced, where svr_get_stats raises if a triangle the test would
drop wins a pixel.  Each frame must be the oracle's, bit for bit."""
import pytest

import scenarios as SC
import svr_testlib as T

A = SC.A
pytestmark = pytest.mark.gpu

TUNE_NO_SPLIT, TUNE_NO_HIZ, TUNE_HIZ = 8, 32, 64  # SVR_OPT_TUNING bits (csrc/svr_device.h)
SETTINGS = {  # name: (instrumented, tuning)
    "auto": (0, 0),
    "no_hiz": (0, TUNE_NO_HIZ),
    "hiz": (0, TUNE_HIZ),
    "hiz_no_split": (0, TUNE_HIZ | TUNE_NO_SPLIT),
    "hiz_instrumented": (1, TUNE_HIZ),
    "no_split_instrumented": (1, TUNE_NO_SPLIT),
}
COUNTS = ("triangle_count", "drawcall_count", "culled_draws")
INSTR_COUNTS = COUNTS + ("rasterized_fragments", "binned_triangles")


def run(lib, name, instrumented, tuning, mp):
    """scenario `name` with its options set right before its draw call"""
    orig = A.Renderer.draw_geometry

    def draw(self, scene, opaque, transparent=None):
        self.set_option(A.OPT_COUNT_FRAGMENTS, instrumented)
        self.set_option(A.OPT_TUNING, tuning)
        return orig(self, scene, opaque, transparent)

    with mp.context() as m:
        m.setattr(A.Renderer, "draw_geometry", draw)
        return SC.SCENARIOS[name](lib)


def test_no_split_bit_is_the_one_launch_tiles_reads():
    import re
    with open(f"{T.ROOT}/simple-vk-renderer_amd/csrc/svr_device.h") as f:
        src = f.read()
    for bit, name in ((TUNE_NO_SPLIT, "TUNE_NO_SPLIT"), (TUNE_NO_HIZ, "TUNE_NO_HIZ"), (TUNE_HIZ, "TUNE_HIZ")):
        m = re.search(rf"constexpr uint32_t {name}\s*=\s*(\d+)u", src)
        assert m and int(m.group(1)) == bit, name


@pytest.mark.parametrize("name", sorted(SC.SCENARIOS))
def test_timed_instances_match_the_oracle(hip, oracle, name, monkeypatch):
    ref = SC.SCENARIOS[name](oracle)  # instrumented: the oracle's frame does not depend on the HIP settings
    for setting, (instrumented, tuning) in SETTINGS.items():
        got = run(hip, name, instrumented, tuning, monkeypatch)
        what = f"{name} {setting}"
        for key in ("color", "depth", "rgba8"):
            T.assert_images_identical(got[key], ref[key], f"{what} {key}")
        for f in (INSTR_COUNTS if instrumented else COUNTS):
            assert getattr(got["stats"], f) == getattr(ref["stats"], f), f"{what}: {f}"
