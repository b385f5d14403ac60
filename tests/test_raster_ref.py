"""The fixed-function stages of the CPU oracle against tests/raster_ref.py, the independent float64 / exact-integer
statement of the rules: coverage at every pixel with no allowance; depth and colour at every covered pixel and b1, b2,
1/w, u, v, the quad derivatives and the fp32 texel (through svr_debug_trace_pixel) at a seeded sample of the covered
pixels, each within the allowance the reference derives for it.  tests/test_raster_ref_gpu.py runs the same cases and
the same checker, check_case, on the HIP library.

Family D adds the clip volume and the guard band (C2), stated by the reference from the definition of the volume.  For
the triangles that go through the clipper, and only for them, check_case learns an either/or band of coverage of
width tau around the ideal boundary (pixels farther than tau must match exactly; the band is capped like the texel's
either/or rule), skips b1, b2 (a piece's, not the parent's), and adds the snap term to the allowances.  Every single
opaque triangle of any family must also report as many rasterised fragments as it covers pixels, the one place a pixel
drawn twice on a fan's diagonal shows; pairs that share a cut edge are disjoint exactly and leave no hole beyond tau of
the union's outer boundary; triangles wholly outside draw nothing.

The reference is also shown to bite: every deliberately wrong variant of it (raster_ref.VARIANTS) must disagree with the
oracle on at least one case, beyond the allowances.

`python tests/test_raster_ref.py` (with the repository root on PYTHONPATH) prints the table of DESIGN.md §2: per
quantity, the oracle's worst error over its allowance, families B and C and then D's clipped triangles, and the worst
distance of a coverage disagreement beside tau."""
import numpy as np
import pytest

import raster_cases as RC
import raster_ref as RR

EPS = RR.EPS
TRACED, EITHER_OR_CAP = RC.TRACED, RC.EITHER_OR_CAP  # (the generator of family D accepts its cases by the same two)
FAMILIES = ("A32", "A40", "B", "C", "D")


class Ratios(dict):
    """worst |error| / allowance per quantity; for clipped triangles also the worst distance (pixels) of a coverage
    disagreement from the ideal boundary, beside the widest band tau met"""
    band_worst = 0.0
    band_tau = 0.0
    band_uses = 0

    def note(self, name, err, tol):
        err, tol = np.asarray(err, np.float64), np.asarray(tol, np.float64)
        if err.size:  # (an exact zero, b = 0 on an edge say, has the allowance 0 and the error 0)
            ratio = np.divide(err, tol, out=np.where(err > 0, np.inf, 0.0), where=tol > 0)
            self[name] = max(self.get(name, 0.0), float(ratio.max()))


def _fail(case, what, k, ref, got, want, tol):
    raise AssertionError(f"{case.name}: {what} at pixel (x, y) = ({int(ref.xs[k])}, {int(ref.ys[k])}): got {np.asarray(got).tolist()}, "
                         f"the reference says {np.asarray(want).tolist()} +- {np.asarray(tol).tolist()}")


def _check_scalar(case, ref, name, ks, got, ratios, what=None):
    want, tol = ref.val[name][ks], ref.tol[name][ks]
    err = np.abs(got.astype(np.float64) - want)
    ratios.note(what or name, err, tol)
    bad = ~(err <= tol)
    if bad.any():
        i = int(np.argmax(bad))
        _fail(case, what or name, ks[i], ref, got[i], want[i], tol[i])


def _check_texel(case, ref, ks, got, extra, ratios, what):
    """got (n, C <= 4) against the texel, allowance + extra (n, C); the either/or rule where the reference offers it.
    -> the pixels (indices into ks) that passed on an alternative only"""
    c = got.shape[1]
    want, tol = ref.val["texel"][ks][:, :c], ref.tol["texel"][ks][:, :c] + extra
    err = np.abs(got.astype(np.float64) - want)
    ok = np.all(err <= tol, axis=1)
    ratios.note(what, err[ok], tol[ok])
    used = []
    for i in np.nonzero(~ok)[0]:
        alts = ref.alts.get(int(ks[i]), [])
        if not any(np.all(np.abs(got[i].astype(np.float64) - v[:c]) <= t[:c] + extra[i]) for v, t in alts):
            _fail(case, what + (f" ({len(alts)} alternatives offered)" if alts else ""), ks[i], ref, got[i], want[i], tol[i])
        used.append(i)
    return used


def half_fp16_ulp(v):
    """half an fp16 ulp of |v| (of the next larger fp16 value, so that a result rounded upwards is covered)"""
    h = np.abs(v).astype(np.float16)
    return 0.5 * np.spacing(np.nextafter(h, np.float16(np.inf))).astype(np.float64)


class _Cut:
    pass


def _restrict(ref, keep):
    """the reference's per-pixel arrays at the covered pixels `keep` (bool over them) only"""
    out = _Cut()
    out.__dict__.update(ref.__dict__)
    idx = np.nonzero(keep)[0]
    remap = {int(k): i for i, k in enumerate(idx)}
    out.ys, out.xs, out.clipped, out.ambiguous = ref.ys[idx], ref.xs[idx], ref.clipped[idx], ref.ambiguous[idx]
    out.val = {k: v[idx] for k, v in ref.val.items()}
    out.tol = {k: v[idx] for k, v in ref.tol.items()}
    out.mag = {k: v[idx] for k, v in ref.mag.items()}
    out.alts = {remap[k]: v for k, v in ref.alts.items() if k in remap}
    out.covered = np.zeros_like(ref.covered)
    out.covered[out.ys, out.xs] = True
    return out


def check_case(case, ref, got, ratios=None):
    """One pass of a library against the reference's result of it.  got: "covered", "depth", "color" over the target,
    and either the attribute planes "bary", "uv", "albedo" (every covered pixel is checked) or "pixels" [(x, y)] with
    their "traces" (the oracle), and "fragments" (stats.rasterized_fragments of the pass).  Raises AssertionError on the
    first disagreement; returns the number of covered pixels checked and how many pixels needed an either/or rule (of the
    texel, or of a clipped triangle's coverage band)."""
    ratios = Ratios() if ratios is None else ratios
    # 1. coverage: set equality, no allowance.  Only a triangle that went through the clipper has pixels offered either
    # way, those within tau of its ideal boundary (ref.offered): beyond tau none may be missing and none may be added.
    clipped = case.family == "D" and getattr(case, "clipped", False)
    if not clipped:
        assert not ref.offered.any() and not ref.clipped.any(), f"{case.name}: only the clipper's triangles have a coverage band"
    differ = got["covered"] != ref.covered
    if (differ & ~ref.offered).any():
        d = np.argwhere(differ & ~ref.offered)
        raise AssertionError(f"{case.name}: coverage differs at {len(d)} pixels, first (y, x) = {d[0].tolist()}: "
                             f"library {bool(got['covered'][tuple(d[0])])}, reference {bool(ref.covered[tuple(d[0])])}"
                             + (f", {float(ref.dist[tuple(d[0])]):.5f} px from the ideal boundary, tau = {ref.tau:.5f}" if clipped else ""))
    band_used, band_offered = int(differ.sum()), int(ref.offered.sum())
    assert band_used <= band_offered <= EITHER_OR_CAP * len(ref.ys), \
        f"{case.name}: coverage offered either way at {band_offered} and used at {band_used} of {len(ref.ys)} covered pixels"
    if band_used:
        ratios.band_worst = max(ratios.band_worst, float(ref.dist[differ].max()))
        ratios.band_uses += band_used
    ratios.band_tau = max(ratios.band_tau, ref.tau)
    # a single opaque triangle: every covered pixel is one fragment - a pixel drawn twice (on a fan's diagonal) counts twice
    if len(case.tris) == 1:
        assert got["fragments"] == int(got["covered"].sum()), \
            f"{case.name}: {got['fragments']} fragments rasterised for {int(got['covered'].sum())} covered pixels"
    drawn = got["covered"]
    assert not got["depth"][~drawn].any() and not got["color"][~drawn].any(), f"{case.name}: pixels outside the coverage were written"
    if band_used:  # values are checked where the library and the ideal rule both cover
        ref = _restrict(ref, got["covered"][ref.ys, ref.xs])
    n = len(ref.ys)
    everywhere = np.arange(n)
    if n == 0:
        return 0, band_used
    # 2. depth and colour at every covered pixel.  colour = fp16(texel * c * light) with c = fl(q * fl(1/q)) the
    # interpolated white vertex colour (two roundings), light the same from the normal (two), and two products:
    # 6 roundings + 1 = 7 eps |texel|, then half an fp16 ulp
    _check_scalar(case, ref, "depth", everywhere, got["depth"][ref.ys, ref.xs], ratios)
    rgb = got["color"][ref.ys, ref.xs]
    assert np.all(rgb[:, 3] == 1.0), f"{case.name}: alpha of a covered pixel is not 1"
    t = ref.val["texel"][:, :3]
    used = set(_check_texel(case, ref, everywhere, rgb[:, :3], 7 * EPS * t + half_fp16_ulp(t + ref.tol["texel"][:, :3]), ratios, "colour"))
    # 3. the interpolated quantities and the fp32 texel
    if "bary" in got:
        for plane in ("bary", "uv", "albedo"):
            assert not got[plane][~drawn].any(), f"{case.name}: plane {plane} is not zero where nothing was drawn"
        ks = everywhere
        vals = {"b1": got["bary"][ref.ys, ref.xs, 0], "b2": got["bary"][ref.ys, ref.xs, 1], "r": got["bary"][ref.ys, ref.xs, 2],
                "u": got["uv"][ref.ys, ref.xs, 0], "v": got["uv"][ref.ys, ref.xs, 1]}
        texel, texel_extra = got["albedo"][ref.ys, ref.xs, :3], 4 * EPS * t  # ALBEDO = fl(c * texel): 3 roundings + 1
        assert np.all(got["albedo"][ref.ys, ref.xs, 3] == 1.0) and not got["bary"][ref.ys, ref.xs, 3].any()
    else:
        index = np.full(ref.covered.shape, -1, np.int64)
        index[ref.ys, ref.xs] = everywhere
        ks = np.array([index[y, x] for x, y in got["pixels"]], np.int64)
        tr = got["traces"]
        if clipped:  # (a traced pixel that only the library covers, inside the band, has no reference value)
            tr, ks = tr[ks >= 0], ks[ks >= 0]
        assert np.all(tr[:, 0] != 0.0), f"{case.name}: a traced covered pixel ran no fragment shader"
        vals = {"b1": tr[:, 1], "b2": tr[:, 2], "r": tr[:, 3], "u": tr[:, 4], "v": tr[:, 5]}
        texel, texel_extra = tr[:, 11:15], np.zeros((len(ks), 4))
        err = np.abs(tr[:, 6:10].astype(np.float64) - ref.val["deriv"][ks])
        ratios.note("derivatives", err, ref.tol["deriv"][ks])
        if not np.all(err <= ref.tol["deriv"][ks]):
            i = int(np.argmax(np.any(err > ref.tol["deriv"][ks], axis=1)))
            _fail(case, "derivatives", ks[i], ref, tr[i, 6:10], ref.val["deriv"][ks[i]], ref.tol["deriv"][ks[i]])
    for name, v in vals.items():
        if clipped and name in ("b1", "b2"):  # a piece's, not the parent's: a naming of the libraries' output
            continue
        _check_scalar(case, ref, name, ks, v, ratios)
    used |= {int(ks[i]) for i in _check_texel(case, ref, ks, texel, texel_extra, ratios, "texel")}
    # 4. the either/or rule is capped, and barred from the exact cases
    offered = int(ref.ambiguous.sum())
    if case.exact:
        assert offered == 0 and not used, f"{case.name}: an exact case offers no alternatives"
    assert len(used) <= offered <= EITHER_OR_CAP * n, f"{case.name}: either/or offered at {offered} and used at {len(used)} of {n} covered pixels"
    return n, len(used) + band_used


def check_pair(first, second):
    """two triangles sharing an edge, drawn in a pass each: disjoint, and no hole - every pixel centre strictly inside
    either, or strictly inside the quad on the shared edge, is covered by one of them"""
    a, b = first["covered"], second["covered"]
    assert not (a & b).any(), "a pixel on a shared edge was drawn twice"
    return a | b


def strictly_inside_union(c1, c2, width, height):
    """pixel centres strictly inside triangle 1 or 2, or on the open shared edge (the two vertices both have)"""
    py, px = np.mgrid[0:height, 0:width].astype(np.int64)
    px, py = px * 256 + 128, py * 256 + 128
    shared = [p for p in c1.grid if p in c2.grid]
    out = np.zeros((height, width), bool)
    for c in (c1, c2):
        v = c.grid
        s = RR._cross(*v[0], *v[1], *v[2])
        if s == 0:
            continue
        inside, on_shared = np.ones((height, width), bool), np.ones((height, width), bool)
        for i in range(3):
            a, b = v[(i + 1) % 3], v[(i + 2) % 3]
            e = RR._cross(*a, *b, px, py) * (1 if s > 0 else -1)
            inside &= e > 0
            on_shared &= (e == 0) if (a in shared and b in shared) else (e > 0)
        out |= inside | on_shared
    return out


# ---------------------------------------------------------------- the oracle's passes, made once
_ORACLE = {}


def oracle_results(oracle, family):
    if family not in _ORACLE:
        cases = RC.cases(family)
        rigs = {}
        rng = np.random.default_rng(515)
        out = []
        for case in cases:
            if (case.width, case.height) not in rigs:
                rigs[(case.width, case.height)] = RC.Rig(oracle, case.width, case.height)
            rig = rigs[(case.width, case.height)]
            got = rig.draw(case)
            ys, xs = np.nonzero(got["covered"])
            if case.family != "A" and len(ys):
                pick = rng.choice(len(ys), min(TRACED, len(ys)), replace=False)
                got = rig.draw(case, [(xs[i], ys[i]) for i in pick])
                got["pixels"] = [(int(xs[i]), int(ys[i])) for i in pick]
            else:
                got["pixels"], got["traces"] = [], np.zeros((0, 64), np.float32)
            out.append(got)
        for rig in rigs.values():
            rig.close()
        _ORACLE[family] = out
    return _ORACLE[family]


RATIOS = Ratios()


def run_family(results, family, ratios, only_clipped=False):
    """every case of a family through check_case; -> (cases, covered pixels, either/or uses).  only_clipped: the ratios
    of family D's controls, which keep the exact path, are left out of `ratios`"""
    cases = RC.cases(family)
    total = used = 0
    for k, (case, got) in enumerate(zip(cases, results)):
        n, u = check_case(case, RC.reference(case), got, Ratios() if only_clipped and not case.clipped else ratios)
        total, used = total + n, used + u
        check_pair_of(cases, k, results[k - 1] if k else None, got)
        if case.family != "A" and not getattr(case, "empty", False):
            assert n >= TRACED, f"{case.name}: covers {n} pixels only"
        if getattr(case, "empty", False):
            assert n == 0 and not got["covered"].any() and got["fragments"] == 0, f"{case.name}: something was drawn"
    return len(cases), total, used


def check_pair_of(cases, k, prev, got):
    """cases[k], if it is the second of a pair: disjoint from the first exactly, and no hole.  Family A: every centre
    strictly inside the quad.  Family D, where a plane cuts the shared edge: every ideally covered centre farther than
    tau from the union's OUTER boundary - the shared edge offers nothing, it is cut at the identical vertex (C2)."""
    case = cases[k]
    if not case.pair:
        return
    union = check_pair(prev, got)
    if case.family == "D":
        want = np.zeros_like(union)
        for c in (cases[k - 1], case):
            t = RC.reference(c).tris[0]
            want |= (t.signed_distance() >= 0.0) & (t.signed_distance(skip=(c.opposite,)) > t.tau)
    else:
        want = strictly_inside_union(cases[k - 1], case, case.width, case.height)
    assert not (want & ~union).any(), f"{case.name}: a hole on the shared edge"


@pytest.mark.parametrize("family", FAMILIES)
def test_oracle_against_the_reference(oracle, family):
    n_cases, total, used = run_family(oracle_results(oracle, family), family, RATIOS)
    print(f"{family}: {n_cases} cases, {total} covered pixels, either/or used at {used}")
    assert total > 0


def test_allowances_stay_within_16_eps_of_their_magnitude_sums(oracle):
    """(for a clipped triangle: the allowance less its snap term, which is no rounding and is listed separately; b1, b2
    are a piece's there and have none)"""
    for family in ("B", "C", "D"):
        oracle_results(oracle, family)  # (reads the mip chains back)
        for case in RC.cases(family):
            ref = RC.reference(case)
            for name in ("b1", "b2", "r", "depth", "u", "v"):
                if not ref.clipped.any():
                    assert np.all(ref.tol[name] <= 16 * EPS * ref.mag[name]), f"{case.name}: the allowance of {name}"
                elif name not in ("b1", "b2"):  # (1e-12: the subtraction's own float64 rounding)
                    assert np.all(ref.tol[name] - ref.snap[name] <= 16 * EPS * ref.mag[name] * (1 + 1e-12)), f"{case.name}: the allowance of {name}"


def test_oracle_error_ratios(oracle):
    """Worst observed error of the oracle over the allowance, per quantity: above 0.5 the derivation (or the reference)
    is wrong, below 0.01 the allowance is too loose to catch anything.  Two quantities cannot keep under 0.5 and have
    bounds of their own.  b1, b2: a chain of only four roundings, allowed 5 eps |b|; four roundings do not average out
    (2.7 eps is observed, 4 eps is possible), so the bound is 4/5.  Colour: its allowance is the half fp16 ulp of the
    store, which any correctly rounded result comes arbitrarily close to: the bound is 1.

    Family D is measured on its own, against the allowances of a clipped triangle.  Those are led by the snap term,
    and a snap of a full 1/512 px in both axes is attainable, so the ceiling of one half does not apply: D's ratios
    are held in [0.01, 1.0]."""
    ratios = Ratios()
    for family in ("B", "C"):
        run_family(oracle_results(oracle, family), family, ratios)
    print({k: round(v, 3) for k, v in ratios.items()})
    for name, v in ratios.items():
        assert 0.01 <= v <= {"b1": 0.8, "b2": 0.8, "colour": 1.0}.get(name, 0.5), f"{name}: worst error / allowance = {v:.4f}"
    clipped = Ratios()
    _, total, used = run_family(oracle_results(oracle, "D"), "D", clipped, only_clipped=True)
    print("D:", {k: round(v, 3) for k, v in clipped.items()}, f"; {total} covered pixels, either/or used at {used}; "
          f"worst coverage disagreement {clipped.band_worst:.5f} px from the ideal boundary, widest tau {clipped.band_tau:.5f} px")
    assert clipped.band_worst <= clipped.band_tau
    for name, v in clipped.items():
        assert 0.01 <= v <= 1.0, f"D {name}: worst error / allowance = {v:.4f}"


VARIANT_FAMILIES = {"bottom_right": ("A32",), "affine_uv": ("B", "D"), "no_near": ("D",), "no_far": ("D",), "behind_the_eye": ("D",),
                    "guard_saturate": ("D",)}


@pytest.mark.parametrize("variant", RR.VARIANTS)
def test_wrong_variant_of_the_reference_is_caught(oracle, variant):
    """on every family listed for it (affine uv: on B, and on D's clipped triangles as well: D's cases that keep the exact
    path are left out for it, so that it is the clipped rule that is shown to bite)"""
    for family in VARIANT_FAMILIES.get(variant, ("C",)):
        caught = []
        results = oracle_results(oracle, family)
        for case, got in zip(RC.cases(family), results):
            if variant == "affine_uv" and family == "D" and not case.clipped:
                continue
            RC.reference(case)  # (the chain is checked by the true rules first)
            RR.WRONG = variant
            try:
                wrong = RR.render(case.tris, case.width, case.height, RC._CHAINS[(case.tex, case.mipmapped)], case.smp, exact=case.exact)
                check_case(case, wrong, got)
            except AssertionError as e:
                caught.append(str(e))
            finally:
                RR.WRONG = None
            if len(caught) >= 3:
                break
        print(f"{variant} on {family}: e.g. {caught[:1]}")
        assert caught, f"the reference with '{variant}' agrees with the oracle on every case of {family}: cases or allowances are too weak"


if __name__ == "__main__":
    import svr_testlib
    lib = svr_testlib.load_oracle()
    table = Ratios()
    for fam in ("B", "C"):
        print(fam, run_family(oracle_results(lib, fam), fam, table))
    for name_, v_ in table.items():
        print(f"| {name_} | {v_:.3f} |")
    table = Ratios()
    print("D", run_family(oracle_results(lib, "D"), "D", table, only_clipped=True))
    for name_, v_ in table.items():
        print(f"| D {name_} | {v_:.3f} |")
    print(f"coverage: worst disagreement {table.band_worst:.5f} px, tau up to {table.band_tau:.5f} px, {table.band_uses} uses")
