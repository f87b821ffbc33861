"""GPU (MI355X): the BSDF and bitmap-texture routines of pt_device.h one call at a time (mi_debug_bsdf / mi_debug_texture, csrc/kernels_units.hip) against the
oracle's orc_bsdf_sample_ex / orc_bsdf_eval / orc_texture_eval on the inputs of tests/unit_inputs.py: directions, sample values and footprints that camera-driven
paths almost never produce.  tests/test_unit_inputs.py checks on the CPU that those inputs reach every lobe and every branch."""
import numpy as np
import pytest
from tests import unit_inputs as U
from tests.test_unit_inputs import texture_properties

pytestmark = pytest.mark.gpu
BIT_SHARE_FLOOR = 0.9999      # the project's floor where csrc/libm_glibc.h is in play (test_gpu_parity.bit_share)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(got, ref):
    """per case: every output equal bit for bit; NaN counts as equal to NaN"""
    return ((bits(got) == bits(ref)) | (np.isnan(got) & np.isnan(ref))).all(1)


def rel_err(got, ref):
    """the `err` of test_gpu_parity.py: largest component difference over the largest reference component"""
    with np.errstate(invalid="ignore"):
        return np.abs(got - ref).max(1) / (np.abs(ref).max(1) + 1e-6)


def oracle_as_device(sampled):
    """orc_bsdf_sample_ex's ten outputs in the device's layout: the component code 0 / 1 / 2 becomes the delta and null flags"""
    return np.concatenate([sampled[:, :8], (sampled[:, 8:9] != 0).astype(np.float32), (sampled[:, 8:9] == 2).astype(np.float32), sampled[:, 9:10]], 1)


def within_tolerance(got, ref, sample):
    """a case that is not bit-equal still meets the project's own tolerances: err < 1e-4 on weight / value and pdf, wo within 2e-5, equal eta and flags, the same zero
    pattern, non-finite exactly where the oracle is non-finite (an infinity with the oracle's sign)"""
    fin = np.isfinite(ref)
    ok = (np.isnan(got) == np.isnan(ref)).all(1) & (np.isinf(got) == np.isinf(ref)).all(1) & (np.where(np.isinf(ref), np.sign(got) == np.sign(ref), True)).all(1)
    ok &= ((got == 0) == (ref == 0)).all(1)
    g, r = np.where(fin, got, 0.0), np.where(fin, ref, 0.0)
    ok &= (rel_err(g[:, 0:3], r[:, 0:3]) < 1e-4) & (rel_err(g[:, 3:4], r[:, 3:4]) < 1e-4)
    if sample: ok &= (np.abs(g[:, 4:7] - r[:, 4:7]).max(1) <= 2e-5) & (got[:, 7] == ref[:, 7]) & (got[:, 8:11] == ref[:, 8:11]).all(1)
    return ok


@pytest.fixture(scope="module")
def bsdf_runs(mi, oracle, golden_scenes):
    """every unrefused record of every scene through the device, once: rows of (scene, record, type, mode, inputs, device outputs, oracle outputs)"""
    runs = []
    for name in U.BSDF_SCENES:
        sc = golden_scenes[name]; ref = U.bsdf_reference(oracle, golden_scenes, name); gs = mi.Scene(sc)
        for m, r in ref.items():
            inp = r["inp"]
            runs.append(dict(scene=name, record=m, type=sc.bsdfs[m]["type"], exact=U.no_libm(sc, m), mode="sample", got=gs.bsdf_units(m, inp["wi"], uv=inp["uv"], extra=inp["extra"]),
                             ref=oracle_as_device(r["sampled"]), inputs=np.concatenate([inp["wi"], inp["uv"], inp["extra"][:, None]], 1)))
            runs.append(dict(scene=name, record=m, type=sc.bsdfs[m]["type"], exact=U.no_libm(sc, m), mode="eval", got=gs.bsdf_units(m, inp["wi"], wo=r["wo"]),
                             ref=r["evald"], inputs=np.concatenate([inp["wi"], r["wo"]], 1)))
        gs.close()
    return runs


def describe(run, i):
    return f"{run['scene']} record {run['record']} ({U.TYPE_NAMES[run['type']]}) {run['mode']} case {i}: in {run['inputs'][i].tolist()} device {run['got'][i].tolist()} oracle {run['ref'][i].tolist()}"


@pytest.mark.parametrize("name", U.BSDF_SCENES)
def test_bsdf_units_without_libm(bsdf_runs, name):
    """diffuse, conductor, dielectric, thindielectric, plastic, difftrans, null and mixtures / blends of them: their device code calls no math-library routine, so
    every output of every case equals the oracle's bit for bit"""
    for run in bsdf_runs:
        if run["scene"] != name or not run["exact"]: continue
        eq = same(run["got"], run["ref"])
        for i in np.flatnonzero(~eq)[:8]: print("[unit-bsdf] " + describe(run, i))
        assert eq.all(), (name, run["record"], run["mode"], float(eq.mean()))


def test_bsdf_units_with_libm(bsdf_runs):
    """every other type, pooled per BSDF type over all scenes: at least 0.9999 of the cases equal the oracle in every output bit; every case outside that share is
    printed and still meets the project's tolerances"""
    pools = {}
    for run in bsdf_runs:
        if run["exact"]: continue
        eq = same(run["got"], run["ref"]); tol = within_tolerance(run["got"], run["ref"], run["mode"] == "sample")
        for i in np.flatnonzero(~eq): print("[unit-bsdf] " + ("" if tol[i] else "OUT OF TOLERANCE ") + describe(run, i))
        p = pools.setdefault(U.TYPE_NAMES[run["type"]], dict(n=0, eq=0, bad=0)); p["n"] += len(eq); p["eq"] += int(eq.sum()); p["bad"] += int((~eq & ~tol).sum())
    assert pools
    for t, p in sorted(pools.items()): print(f"[bit-share] unit {t}: {p['eq'] / p['n']:.6f} of {p['n']} cases, {p['bad']} outside the tolerances")
    for t, p in pools.items():
        assert p["bad"] == 0 and p["eq"] / p["n"] >= BIT_SHARE_FLOOR, (t, p)


def test_bsdf_units_refusals(mi, golden_scenes):
    """records that need a hit record are refused by name (MI_ERR_UNSUPPORTED = 3): the path-level tests stay their cover"""
    seen = set(); wi = np.array([[0.0, 0.0, 1.0]], np.float32)
    for name in ("masked_room", "layered_room", "bitmap_room"):
        sc = golden_scenes[name]; gs = mi.Scene(sc)
        for m, b in enumerate(sc.bsdfs):
            if not U.refused(sc, m): continue
            kind = "mask" if b["type"] == 9 else "bumpmap" if b["type"] == 11 else "normalmap" if b["type"] == 12 else "bound texture" if b.get("texture", -1) >= 0 else None
            for kw in (dict(wo=wi), dict(uv=[[0.5, 0.5]])):
                with pytest.raises(mi.MiError) as e: gs.bsdf_units(m, wi, **kw)
                assert e.value.code == 3 and (kind is None or kind in str(e.value)), str(e.value)
            seen.add(kind)
        gs.close()
    assert {"mask", "bumpmap", "normalmap", "bound texture"} <= seen


@pytest.fixture(scope="module")
def texture_runs(mi, oracle):
    """the texture scene committed once; per record the device's filtered lookups (only those whose EWA loops the CPU census found short) and its plain ones"""
    sc, orc, per = U.texture_reference(oracle, mi.scenes)
    assert np.mean([(~p["keep"]).mean() for p in per.values()]) <= 0.001      # the cap of test_unit_inputs' census, checked again before any launch
    gs = mi.Scene(sc); out = {}
    for t, p in per.items():
        k = p["keep"]
        out[t] = dict(keep=k, filtered=gs.texture_units(t, p["uv"][k], p["pa"][k]), ref=p["ref"][k], plain=gs.texture_units(t, p["uv"]), ref_plain=p["plain"], uv=p["uv"][k], pa=p["pa"][k])
    yield sc, gs, out
    gs.close()


def test_texture_units_exact(texture_runs):
    """nearest, bilinear, the route without partials and the procedural textures: bit for bit"""
    sc, gs, out = texture_runs
    for t, r in out.items():
        eq = same(r["plain"], r["ref_plain"]); assert eq.all(), (t, "plain", float(eq.mean()), r["uv"][~eq][:4])
        if sc.textures[t]["type"] != 2 or sc.textures[t]["filter"] < 2:
            eq = same(r["filtered"], r["ref"])
            for i in np.flatnonzero(~eq)[:8]: print(f"[unit-texture] record {t} case {i}: uv {r['uv'][i].tolist()} partials {r['pa'][i].tolist()} device {r['filtered'][i].tolist()} oracle {r['ref'][i].tolist()}")
            assert eq.all(), (t, float(eq.mean()))


@pytest.mark.parametrize("f", [2, 3])
def test_texture_units_filtered(texture_runs, f):
    """trilinear and EWA: the level comes from a logarithm, the clamped ellipse from atan / sin / cos (csrc/libm_glibc.h).  Bit share >= 0.9999 per filter; the rest
    within err < 1e-4 -- both filters are continuous across a level boundary, so a last-bit difference of the logarithm cannot exceed that"""
    sc, gs, out = texture_runs; n = eq_n = 0
    for t, r in out.items():
        if sc.textures[t]["type"] != 2 or sc.textures[t]["filter"] != f: continue
        eq = same(r["filtered"], r["ref"]); err = rel_err(r["filtered"], r["ref"])
        for i in np.flatnonzero(~eq): print(f"[unit-texture] record {t} case {i}: uv {r['uv'][i].tolist()} partials {r['pa'][i].tolist()} device {r['filtered'][i].tolist()} oracle {r['ref'][i].tolist()} err {err[i]:.3g}")
        assert (np.isfinite(r["filtered"]) == np.isfinite(r["ref"])).all() and (err[~eq] < 1e-4).all(), (t, float(np.nanmax(err)))
        n += len(eq); eq_n += int(eq.sum())
    print(f"[bit-share] unit texture {U.FILTER_NAMES[f]}: {eq_n / n:.6f} of {n} lookups")
    assert eq_n / n >= BIT_SHARE_FLOOR


def test_texture_units_properties(texture_runs):
    """stored texels at texel centres, the nearest filter's index rule under all five wrap modes, the constant bitmap: on the device, without the oracle"""
    sc, gs, out = texture_runs
    texture_properties(lambda t, uv, pa: gs.texture_units(t, uv, pa), sc, keep={t: r["keep"] for t, r in out.items()})
