"""The fragment stage's third cut, on the host (csrc/svr_device.h): tests/native/frag_third_check.cpp compiles the header's own
code -- the binding's LOD clamps (binding_min_lod, LOD_SELECT, binding_lod_range), lod_from_rho2 in both forms and edge_bias, cut
out of the header the way tests/test_frag_setup.py cuts its helpers -- under the address and undefined-behaviour sanitizers, and
checks

  * clamp_med3(lod_from_rho2<false>(x), lo, hi) against clamp_med3(lod_from_rho2<true>(x), lo, hi), bit for bit, for every
    exponent field (the NaNs' too) x 2^16 evenly spaced mantissas, every float within 2048 ulps of 2^100 and 2^-100, 0, the
    denormals' ends, FLT_MAX and +inf, under (lo, hi) in {(-50, 50), (0, 0), (0, 10), (3.5, 3.5), (-50, -50), (50, 50)};
  * that binding_lod_range changes no clamp of a value in [-50, 50] and calls a range wide exactly when it lies outside;
  * that with edges 1 and 2 stored unbiased, f = g - u and g are the doubles the biased record gave as f and f + u, for seeded
    integer edges with |A|, |B| <= 2^29, |C| < 2^52, pixels in [-2^15, 2^15] and constructed ties g = 0, -1, 1 under either
    bias; that "g >= u" is "f >= 0"; and that the bias read off an edge's steps is the top-left rule's.

CPU only."""
import os
import subprocess

import __graft_entry__ as g
import native_ref as N

HEADER = os.path.join(g.PKG_DIR, "csrc", "svr_device.h")
CUTS = (("// The lower LOD clamp a binding carries", "// Range proofs of the common-case fragment stage", ("binding_min_lod", "binding_lod_range")),
        ("// u_i of TriRec::C above", "struct ClipItem", ("edge_bias",)),
        ("// C10: lambda = log2(rho)", "// 1.0f / x, correctly rounded", ("lod_from_rho2",)))


def third_cut_helpers():
    text = open(HEADER).read()
    parts = []
    for first, last, names in CUTS:
        body = text[text.index(first):text.index(last)]
        for name in names:
            assert f" {name}(" in body, name
        parts.append(body)
    assert "LOD_SELECT = 50.0f" in parts[0] and "template <bool SELECTS" in parts[2]
    return "\n".join(parts)


def test_lod_forms_and_unbiased_edges(tmp_path):
    (tmp_path / "frag_third_under_test.h").write_text(third_cut_helpers())
    exe = N.build("frag_third_check", include=(str(tmp_path),), extra=("-Wall",), sanitize=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    words = r.stdout.split()
    assert words[-1] == "ok", r.stdout
    assert int(words[words.index("lod") + 1]) >= 6 * (255 * 65536 + 12 + 2 * 4096), r.stdout
    assert int(words[words.index("ranges") + 1]) > 100 * 801 and int(words[words.index("edges") + 1]) > 3_000_000, r.stdout
