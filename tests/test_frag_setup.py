"""What the fragment stage's common case takes from setup, on the host (csrc/svr_device.h): tests/native/frag_setup_check.cpp
compiles the header's own helpers — tex_consts, the packed_* forms and frag_ranges_ok, cut out of it between the TexBinding and
TriRec definitions, so the test runs the code the kernels run — and checks that the packed-constant forms equal the closed
forms for every lw, lh in 0..14 and every level, that no triangle the predicate calls common has a covered pixel outside the
reciprocal's window or with |u|, |v| >= 2^23 (a walk over every covered pixel, fp32 chain by std::fmaf), and that the predicate
keeps at least 99 % of the ordinary-camera family.  CPU only."""
import os
import subprocess

import __graft_entry__ as g
import native_ref as N

HEADER = os.path.join(g.PKG_DIR, "csrc", "svr_device.h")


def setup_helpers():
    text = open(HEADER).read()
    first = text.index("constexpr uint32_t TEX_TILE_LW")
    last = text.index("// A set-up triangle, 256 bytes")
    body = text[first:last]
    for name in ("tex_consts", "packed_level_lw", "packed_level_lh", "packed_level_bytes", "packed_mip_offset", "frag_ranges_ok"):
        assert f" {name}(" in body, name
    return "#include <cstdint>\nnamespace svr_layout {\n" + body + "}\n"


def test_packed_constants_and_range_proofs(tmp_path):
    (tmp_path / "frag_setup_under_test.h").write_text(setup_helpers())
    exe = N.build("frag_setup_check", include=(str(tmp_path),), extra=("-Wall",), sanitize=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    words = r.stdout.split()
    assert words[-1] == "ok", r.stdout
    assert int(words[words.index("consts") + 1]) > 15 * 15 * 4 and int(words[words.index("pixels") + 1]) > 100000, r.stdout
    assert float(words[words.index("keep") + 1]) >= 0.99, r.stdout
