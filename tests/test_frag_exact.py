"""The exact identities the common-case fragment stage is spelled with (csrc/k_tile.hip shade_pixel, DESIGN.md section 5 phase B):
extents as exponents (ldexpf for the product with a power of two), clamps as medians over a pair make_binding has put in order
(csrc/svr_device.h binding_min_lod, the header's own code, cut out as tests/test_frag_setup.py cuts it), derivatives without
their parity selects, and the quad partners' edge values by a flipped sign bit instead of fma(+-1, A, e).
tests/native/frag_exact_check.cpp checks each over its ends and over more than 10^7 seeded values, built with the address and
undefined-behaviour sanitizers.  CPU only."""
import subprocess

import native_ref as N
import test_frag_setup as host


def test_exact_identities(tmp_path):
    text = host.setup_helpers()
    assert " binding_min_lod(" in text
    (tmp_path / "frag_setup_under_test.h").write_text(text)
    exe = N.build("frag_exact_check", include=(str(tmp_path),), extra=("-Wall",), sanitize=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    words = r.stdout.split()
    assert words[-1] == "ok", r.stdout
    count = lambda name: int(words[words.index(name) + 1])
    assert count("scalings") > 2 * 10**7 and count("medians") > 10**7 and count("derivatives") > 10**6 and count("partners") > 10**6, r.stdout
