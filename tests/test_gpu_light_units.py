"""GPU (MI355X): the emitter and medium routines of pt_device.h one call at a time (mi_debug_emitter_sample / mi_debug_emitter_eval / mi_debug_medium,
csrc/kernels_units.hip) against the oracle's orc_emitter_sample_units / orc_emitter_eval_units / orc_medium_units on the inputs of tests/unit_inputs.py: reference points, sample values and directions that camera-driven paths
almost never produce.  tests/test_unit_inputs.py checks on the CPU that those inputs reach every branch."""
import numpy as np
import pytest
from tests import unit_inputs as U
from tests.test_gpu_units import BIT_SHARE_FLOOR, bits, rel_err, same, within_tolerance
from tests.test_unit_inputs import LIGHT_ALL, MEDIUM_ALL

pytestmark = pytest.mark.gpu
VALUE_PDF = [0, 1, 2, 10]                        # of the 17 outputs of a sample: value rgb and density
EXACT_KINDS = ["area_mesh", "area_analytic", "point", "directional", "constant", "collimated"]      # device code: arithmetic, sqrtf, the restated sincosf / sincos2pi
LIBM_KINDS = ["spot", "envmap"]                  # acosf; sinf / cosf, and atan2f / acosf on the evaluation side (csrc/libm_glibc.h)


def default_search_flags(sc):
    """DScene::search_flags as the commit derives them: bit 0 = at most three emitters, bit 1 = at most three triangles in every light mesh"""
    tris = [len(ts) for _, ts in U._mesh_lights(sc)]
    return (1 if len(sc.emitters) <= 3 else 0) | (2 if max(tris, default=0) <= 3 else 0)


def routes(sc, name):
    """the values of MI355PT_SEARCH a scene is committed under: None (the default) and, where the default fetches a table whole, "0" (the loops).  The unit scenes also
    take "3": their three-triangle mesh sits next to one of five triangles, so by default its table is searched by the loop."""
    return [None] + (["0"] if default_search_flags(sc) else []) + (["3"] if name in U.UNIT_LIGHT_SCENES else [])


@pytest.fixture(scope="module")
def light_runs(mi, oracle, golden_scenes):
    """every scene through the device once per search route: name -> dict(ref = the oracle's side, routes = {route: dict(sample, raw, eval = {emitter: out})})"""
    runs = {}
    for name in LIGHT_ALL:
        ref = U.light_reference(oracle, golden_scenes, mi.scenes, name); sc = ref["sc"]; inp = ref["sample"]["inp"]; per = {}
        for route in routes(sc, name):
            mp = pytest.MonkeyPatch()
            if route is None: mp.delenv("MI355PT_SEARCH", raising=False)
            else: mp.setenv("MI355PT_SEARCH", route)                 # read when the scene is committed
            try:
                gs = mi.Scene(sc)
            finally:
                mp.undo()
            ev = {e: gs.emitter_eval_units(e, r["inp"]["ref"], r["inp"]["d"], r["inp"]["n"], r["inp"]["dist"], r["inp"]["facing"]) for e, r in ref["eval"].items()}
            per[route] = dict(sample=gs.emitter_sample_units(inp["ref"], inp["ref_n"], inp["uv"]), raw=gs.emitter_sample_units(inp["ref"], inp["ref_n"], inp["uv"], raw=True), eval=ev)
            gs.close()
        runs[name] = dict(ref=ref, routes=per)
    return runs


def kind_of(oracle, branches):
    """per case the emitter kind the oracle's search chose, as a name out of EXACT_KINDS + LIBM_KINDS"""
    B = oracle.Oracle.EMITTER_BRANCHES; out = np.array([""] * len(branches), dtype=object)
    for k in EXACT_KINDS + LIBM_KINDS: out[(branches & B[k]) != 0] = k
    assert (out != "").all()
    return out


def sample_same(got, ref):
    """per case: all 17 outputs equal bit for bit where the oracle returns a density; where it is 0 the oracle leaves the rest of its record unset, and value and
    density alone are compared"""
    lit = ref[:, 10] != 0
    return np.where(lit, same(got, ref), same(got[:, VALUE_PDF], ref[:, VALUE_PDF]))


def sample_within_tolerance(got, ref):
    """a sample that is not bit-equal still meets within_tolerance (value and density err < 1e-4, d within 2e-5, equal emitter index and flags, the same zero and
    non-finite pattern), and p, dist and n agree to the same err"""
    cols = lambda a: np.concatenate([a[:, 0:3], a[:, 10:11], a[:, 6:9], a[:, 14:15], a[:, 15:16], np.zeros((len(a), 2), np.float32)], 1)
    lit = ref[:, 10] != 0; g = np.where(lit[:, None], got, 0.0).astype(np.float32); g[:, VALUE_PDF] = got[:, VALUE_PDF]
    r = np.where(lit[:, None], ref, 0.0).astype(np.float32); r[:, VALUE_PDF] = ref[:, VALUE_PDF]
    ok = within_tolerance(cols(g), cols(r), True)
    with np.errstate(invalid="ignore"):
        ok &= (np.isfinite(g) == np.isfinite(r)).all(1) & ~(rel_err(g[:, 3:6], r[:, 3:6]) >= 1e-4) & ~(rel_err(g[:, 9:10], r[:, 9:10]) >= 1e-4) & ~(np.abs(g[:, 11:14] - r[:, 11:14]).max(1) > 2e-5)
    return ok


def env_texel(sc, d):
    """the texel position (px, py) a world direction maps to in the environment map: what internalSampleDirection drew before its sines and cosines"""
    m = np.asarray(sc.envmap["to_world"], np.float64).reshape(4, 4)[:3, :3]; l = np.asarray(d, np.float64) @ m; h, w = sc.envmap["rgb"].shape[:2]      # (a rotation: its inverse is its transpose)
    return (np.arctan2(l[0], -l[2]) / (2 * np.pi) % 1.0) * w - 0.5, np.arccos(np.clip(l[1], -1, 1)) / np.pi * h - 0.5


def describe(name, route, inp, i, got, ref, kind):
    return f"{name} route {route} case {i} ({kind}): ref {inp['ref'][i].tolist()} n {inp['ref_n'][i].tolist()} uv {inp['uv'][i].tolist()} device {got[i].tolist()} oracle {ref[i].tolist()}"


@pytest.mark.parametrize("name", LIGHT_ALL)
def test_emitter_sample_exact(light_runs, oracle, name):
    """area lights on meshes and on the four analytic shapes, point, directional, constant and the collimated entry: their device code calls nothing but arithmetic,
    sqrtf and the restated sincosf / sincos2pi, so every output of every case equals the oracle's bit for bit -- under every search route; the emitter index, the
    delta flag and em_pdf of the other kinds too"""
    run = light_runs[name]; s = run["ref"]["sample"]; kind = kind_of(oracle, s["branches"]); exact = np.isin(kind, EXACT_KINDS)
    for route, r in run["routes"].items():
        for got, ref, what in ((r["sample"], s["out"], "sample"), (r["raw"], s["raw"], "raw")):
            eq = sample_same(got, ref)
            for i in np.flatnonzero(~eq & exact)[:8]: print("[unit-emitter] " + describe(name, route, s["inp"], i, got, ref, kind[i]))
            assert eq[exact].all(), (name, route, what, float(eq[exact].mean()))
            lit = ref[:, 10] != 0
            assert (bits(got[:, 14:17]) == bits(ref[:, 14:17]))[lit].all(), (name, route, what)


def test_emitter_sample_with_libm(light_runs, oracle):
    """spot (acosf) and envmap (sinf, cosf), pooled per kind over all scenes and routes: at least 0.9999 of the cases equal the oracle in every output bit; every case
    outside that share is printed -- an environment sample with the texel it landed in -- and still meets the project's tolerances"""
    pools = {}
    for name, run in light_runs.items():
        s = run["ref"]["sample"]; kind = kind_of(oracle, s["branches"]); sc = run["ref"]["sc"]
        for route, r in run["routes"].items():
            for got, ref in ((r["sample"], s["out"]), (r["raw"], s["raw"])):
                eq = sample_same(got, ref); tol = sample_within_tolerance(got, ref)
                for k in LIBM_KINDS:
                    mine = kind == k
                    if not mine.any(): continue
                    for i in np.flatnonzero(mine & ~eq):
                        note = ""
                        if k == "envmap" and ref[i, 10] != 0 and got[i, 10] != 0:
                            a, b = env_texel(sc, got[i, 6:9]), env_texel(sc, ref[i, 6:9]); moved = (np.floor(a[0]) != np.floor(b[0])) or (np.floor(a[1]) != np.floor(b[1]))
                            note = f" texel device ({a[0]:.4f}, {a[1]:.4f}) oracle ({b[0]:.4f}, {b[1]:.4f})" + (" DIFFERS BY A TEXEL" if moved else "")
                        print("[unit-emitter] " + ("" if tol[i] else "OUT OF TOLERANCE ") + describe(name, route, s["inp"], i, got, ref, k) + note)
                    p = pools.setdefault(k, dict(n=0, eq=0, bad=0)); p["n"] += int(mine.sum()); p["eq"] += int(eq[mine].sum()); p["bad"] += int((~eq & ~tol & mine).sum())
    assert set(pools) == set(LIBM_KINDS)
    for k, p in sorted(pools.items()): print(f"[bit-share] unit emitter sample {k}: {p['eq'] / p['n']:.6f} of {p['n']} cases, {p['bad']} outside the tolerances")
    for k, p in pools.items(): assert p["bad"] == 0 and p["eq"] / p["n"] >= BIT_SHARE_FLOOR, (k, p)


@pytest.mark.parametrize("name", LIGHT_ALL)
def test_emitter_eval_exact(light_runs, name):
    """what a BSDF-sampled ray that finds an area light evaluates -- Emitter::eval and Scene::pdfEmitterDirect, mesh and analytic shapes alike -- and the constant
    environment's value: bit for bit"""
    run = light_runs[name]; sc = run["ref"]["sc"]
    for route, r in run["routes"].items():
        for e, got in r["eval"].items():
            if sc.emitters[e]["type"] == 1: continue
            ref = run["ref"]["eval"][e]["out"]; eq = same(got, ref); inp = run["ref"]["eval"][e]["inp"]
            for i in np.flatnonzero(~eq)[:8]: print(f"[unit-emitter] {name} route {route} eval emitter {e} case {i}: " + " ".join(f"{k} {inp[k][i].tolist()}" for k in inp) + f" device {got[i].tolist()} oracle {ref[i].tolist()}")
            assert eq.all(), (name, route, e, float(eq.mean()))


def test_envmap_eval_with_libm(light_runs):
    """evalEnvironment and the solid-angle density of EnvironmentMap::pdfDirect (atan2f, acosf), pooled over all environment maps: bit share >= 0.9999, the rest
    printed and within the project's tolerances"""
    n = eq_n = bad = 0
    for name, run in light_runs.items():
        sc = run["ref"]["sc"]
        for e, r in run["ref"]["eval"].items():
            if sc.emitters[e]["type"] != 1: continue
            got = run["routes"][None]["eval"][e][:, :4]; ref = r["out"][:, :4]; eq = same(got, ref); tol = within_tolerance(got, ref, False)
            for i in np.flatnonzero(~eq): print(f"[unit-emitter] {'' if tol[i] else 'OUT OF TOLERANCE '}{name} envmap eval case {i}: d {r['inp']['d'][i].tolist()} device {got[i].tolist()} oracle {ref[i].tolist()}")
            n += len(eq); eq_n += int(eq.sum()); bad += int((~eq & ~tol).sum())
    print(f"[bit-share] unit emitter eval envmap: {eq_n / n:.6f} of {n} cases, {bad} outside the tolerances")
    assert n >= 6 * U.N_LIGHT // 3 and bad == 0 and eq_n / n >= BIT_SHARE_FLOOR


def test_env_eval_and_pdf_is_both_routines(light_runs):
    """envEvalAndPdf equals envEval and envPdfDirection of the same direction bit for bit: a property of the device alone, no share"""
    seen = 0
    for name, run in light_runs.items():
        sc = run["ref"]["sc"]
        for route, r in run["routes"].items():
            for e, got in r["eval"].items():
                if sc.emitters[e]["type"] != 1: continue
                eq = same(got[:, 4:8], got[:, 0:4]); seen += len(eq)
                assert eq.all(), (name, route, got[~eq][:4], run["ref"]["eval"][e]["inp"]["d"][~eq][:4])
    assert seen > 0


def test_search_routes_agree(light_runs):
    """the whole-table fetch and the binary search give the same outputs bit for bit, every field of the record included, on every scene where they differ in route"""
    compared = 0
    for name, run in light_runs.items():
        base = run["routes"][None]
        for route, r in run["routes"].items():
            if route is None: continue
            for what in ("sample", "raw"):
                eq = same(r[what], base[what]); assert eq.all(), (name, route, what, np.flatnonzero(~eq)[:8], run["ref"]["sample"]["inp"]["uv"][~eq][:8])
            for e in r["eval"]: assert same(r["eval"][e], base["eval"][e]).all(), (name, route, e)
            compared += 1
    assert compared >= len(U.UNIT_LIGHT_SCENES) * 2 + 5


def test_emitter_sample_raw(light_runs):
    """raw = 1 (the volumetric integrators' form) is raw = 0 with the value not yet divided by the selection probability: value * (1.0f / em_pdf), one rounding;
    everything else is the same record (that em_pdf equals the oracle's is part of test_emitter_sample_exact)"""
    for name, run in light_runs.items():
        for route, r in run["routes"].items():
            got, raw = r["sample"], r["raw"]; lit = got[:, 10] != 0
            assert same(raw[:, 3:16], got[:, 3:16]).all() and (got[:, 16] == 0).all() and (raw[lit, 16] > 0).all(), (name, route)
            assert same(raw[lit, :3] * (np.float32(1) / raw[lit, 16:17]), got[lit, :3]).all() and (raw[~lit, :3] == 0).all(), (name, route)


def test_emitter_units_refusals(mi, golden_scenes):
    """delta lights are refused by name (MI_ERR_UNSUPPORTED = 3): no ray finds one; an emitter index out of range and an empty batch are MI_ERR_INVALID = 1"""
    one = np.zeros((1, 3), np.float32); up = np.array([[0.0, 1.0, 0.0]], np.float32); seen = set()
    for name in ("cbox_collimated", "open_constant"):
        sc = golden_scenes[name]; gs = mi.Scene(sc)
        for e, em in enumerate(sc.emitters):
            if em["type"] in (0, 1, 2): continue
            with pytest.raises(mi.MiError) as err: gs.emitter_eval_units(e, one, up, up, [1.0], [1.0])
            assert err.value.code == 3 and U.EMITTER_KIND_NAMES[em["type"]] in str(err.value), str(err.value)
            seen.add(U.EMITTER_KIND_NAMES[em["type"]])
        with pytest.raises(mi.MiError) as err: gs.emitter_eval_units(len(sc.emitters), one, up, up, [1.0], [1.0])
        assert err.value.code == 1 and f"of {len(sc.emitters)}" in str(err.value)
        for call in (lambda: gs.emitter_sample_units(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 2))), lambda: gs.emitter_eval_units(0, np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)), [], [])):
            with pytest.raises(mi.MiError) as err: call()
            assert err.value.code == 1
        gs.close()
    assert seen == {"point", "collimated", "spot", "directional"}


# ------------------------------------------------------------------------------------------------ participating media
MEDIUM_BIT_SHARE_FLOOR = 0.999      # the floor of test_volpath_simple where the device library's double exp / log is in play (miFastExp / miFastLog), with rtol 1e-5, atol 1e-7 for the rest


@pytest.fixture(scope="module")
def medium_runs(mi, oracle, golden_scenes):
    """every medium record of every scene through the device once: rows of dict(scene, record, mode, inp, got, ref)"""
    rows = []
    for name in MEDIUM_ALL:
        ref = U.medium_reference(oracle, golden_scenes, mi.scenes, name); gs = mi.Scene(ref["sc"])
        for m, per in ref["records"].items():
            for mode, r in per.items(): rows.append(dict(scene=name, record=m, mode=mode, inp=r["inp"], got=gs.medium_units(m, mode, r["inp"]), ref=r["out"]))
        gs.close()
    return rows


@pytest.mark.parametrize("mode", ["phase_sample", "phase_eval"])
def test_phase_function_exact(medium_runs, mode):
    """phaseSample / phaseEval, isotropic and Henyey-Greenstein on both sides of the |g| < epsilon switch: arithmetic, sqrtf and the polynomial sincos2pi -- bit for bit"""
    seen = 0
    for row in medium_runs:
        if row["mode"] != mode: continue
        eq = same(row["got"], row["ref"]); seen += len(eq)
        for i in np.flatnonzero(~eq)[:8]: print(f"[unit-medium] {row['scene']} record {row['record']} {mode} case {i}: in {row['inp'][i].tolist()} device {row['got'][i].tolist()} oracle {row['ref'][i].tolist()}")
        assert eq.all(), (row["scene"], row["record"], float(eq.mean()))
    assert seen > 0


@pytest.mark.parametrize("mode", ["transmittance", "distance"])
def test_medium_with_double_exp_log(medium_runs, mode):
    """mediumTransmittance and mediumSampleDistance go through the device library's double exp / log: pooled over all records, at least 0.999 of the cases equal the
    oracle in every output bit and the rest lie within rtol 1e-5, atol 1e-7 with NaN where the oracle has NaN; the success flag and the number of values drawn are
    equal in every case"""
    n = eq_n = 0
    for row in medium_runs:
        if row["mode"] != mode: continue
        got, ref = row["got"], row["ref"]; eq = same(got, ref); close = np.isclose(got, ref, rtol=1e-5, atol=1e-7, equal_nan=True).all(1)
        for i in np.flatnonzero(~eq)[:32]: print(f"[unit-medium] {'' if close[i] else 'OUT OF TOLERANCE '}{row['scene']} record {row['record']} {mode} case {i}: in {row['inp'][i].tolist()} device {got[i].tolist()} oracle {ref[i].tolist()}")
        assert close.all(), (row["scene"], row["record"], int((~close).sum()))
        if mode == "distance": assert (got[:, 0] == ref[:, 0]).all() and (got[:, 10] == ref[:, 10]).all(), (row["scene"], row["record"])
        n += len(eq); eq_n += int(eq.sum())
    print(f"[bit-share] unit medium {mode}: {eq_n / n:.6f} of {n} cases")
    assert eq_n / n >= MEDIUM_BIT_SHARE_FLOOR


def test_medium_units_refusals(mi, golden_scenes):
    """a medium index out of range (also on a scene without media), an unknown mode and an empty batch are MI_ERR_INVALID = 1"""
    one = np.zeros((1, 10), np.float32)
    for name, count in (("fog_sky", 2), ("cornell_small", 0)):
        gs = mi.Scene(golden_scenes[name])
        with pytest.raises(mi.MiError) as err: gs.medium_units(count, "transmittance", one)
        assert err.value.code == 1 and f"of {count}" in str(err.value), str(err.value)
        gs.close()
    gs = mi.Scene(golden_scenes["fog_sky"])
    with pytest.raises(mi.MiError) as err: gs.medium_units(0, "distance", np.zeros((0, 10), np.float32))
    assert err.value.code == 1
    assert gs.L.L.mi_debug_medium(gs.h, 0, 4, one.ctypes.data, 1, np.zeros((1, 12), np.float32).ctypes.data) == 1
    gs.close()
