"""Phase A's covered span (csrc/svr_span.h column_span, DESIGN.md section 5 phase A): the rows of a pixel column on which all
three edge functions are >= 0, found once from an fp32 quotient and one exact fp64 test per edge instead of three compares on every
row.  tests/native/column_span_check.cpp compares the header itself with the row-by-row walk it replaces, over more than 10^7
seeded columns and the constructed ties and extremes, each with the reciprocal pushed by -2 .. +2 ulp; built with the address
and undefined-behaviour sanitizers and run directly.
tools/walk_sim.py, the CPU count of the walk the span's gain was estimated with, must reproduce the recorded frame's
rasterised fragments (profiles/frag_diet_bench_ab.txt) to 2 %.  CPU only."""
import os
import subprocess

import pytest

import __graft_entry__ as g
import native_ref as N

RECORDED = {(3840, 2160): 15437085, (1920, 1080): 3858752}  # rasterized_fragments_per_frame, profiles/frag_diet_bench_ab.txt


def test_span_is_the_row_walk():
    exe = N.build("column_span_check", include=(os.path.join(g.PKG_DIR, "csrc"),), extra=("-Wall",), sanitize=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    words = r.stdout.split()
    assert words[-1] == "ok", r.stdout
    count = lambda name: int(words[words.index(name) + 1])
    assert count("random") > 10**7 and count("constructed") > 4 * 10**5, r.stdout
    assert count("runs") == 5 * (count("random") + count("constructed")), r.stdout  # every case under five reciprocals


def test_recorded_counts_are_the_profile_s():
    with open(os.path.join(g.ROOT, "profiles", "frag_diet_bench_ab.txt")) as f:
        text = f.read()
    for (w, h), n in RECORDED.items():
        assert f'"width": {w}, "height": {h}' in text and f'"rasterized_fragments_per_frame": {n},' in text


@pytest.mark.parametrize("size", sorted(RECORDED), ids=lambda s: f"{s[0]}x{s[1]}")
def test_walk_sim_counts_the_recorded_frame(size):
    import importlib.util
    spec = importlib.util.spec_from_file_location("walk_sim", os.path.join(g.ROOT, "tools", "walk_sim.py"))
    sim = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sim)
    r = sim.simulate(*size)
    print(sim.report(r))
    assert abs(r["covered"] - RECORDED[size]) <= 0.02 * RECORDED[size], (r["covered"], RECORDED[size])
    # the walks' bookkeeping: a span is part of its box, pieces of a span cover it, fewer and shorter waves at every stage
    assert r["covered"] <= r["lane_steps"] and r["items_empty"] < r["items"]
    assert r["steps_pieces4"] <= r["steps_pieces8"] <= r["steps_pieces16"] <= r["steps_regrouped"] <= r["steps_span"] <= r["steps_box"]
    assert r["steps_box"] * 64 >= r["lane_steps"] and r["steps_pieces4"] * 64 >= r["covered"]
