"""The texel arena's tiled mip layout on the host (csrc/svr_device.h): tests/native/texel_layout_check.cpp compiles the
header's own layout functions — cut out of it between the TexBinding and TriRec definitions, so the test reads the code
the kernels use, not a copy — and checks, for every extent pair up to 40 x 40 and 1024 x 4, 4 x 1024, 16384 x 1, that
the address function maps each level one-to-one into its own padded span and that levels do not overlap.  CPU only."""
import os
import subprocess

import __graft_entry__ as g
import native_ref as N

HEADER = os.path.join(g.PKG_DIR, "csrc", "svr_device.h")


def layout_functions():
    text = open(HEADER).read()
    first = text.index("constexpr uint32_t TEX_TILE_LW")
    last = text.index("// A set-up triangle, 256 bytes")
    body = text[first:last]
    for name in ("mip_offset", "level_lw", "level_lh", "level_bytes", "texel_offset_x", "texel_offset_y", "texel_offset"):
        assert f" {name}(" in body, name
    return "#include <cstdint>\nnamespace svr_layout {\n" + body + "}\n"


def test_levels_are_bijective_and_disjoint(tmp_path):
    (tmp_path / "texel_layout_under_test.h").write_text(layout_functions())
    exe = N.build("texel_layout_check", include=(str(tmp_path),), extra=("-O1", "-Wall"), sanitize=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    words = r.stdout.split()
    assert words[-1] == "ok" and int(words[1]) > 40 * 40 * 3, r.stdout
