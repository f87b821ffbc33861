"""GPU (MI355X): the surface step between a hit and the BSDF query one hit at a time (mi_debug_surface, csrc/kernels_units.hip) against the oracle's
orc_surface_units on the aimed rays of tests/unit_inputs.py (surface_inputs): tangent selection (surfaceTangents), computePartials and the filtered lookup, the perturbed
frame of bump and normal maps, the unwrap mask -> bump / normal map -> coating with the textured parameters loaded into the nested records, and the query in the resulting
frame.  The device's hits come from mi_debug_intersect_inst on the same rays.  tests/test_surface_inputs.py checks on the CPU that those inputs reach every branch."""
import numpy as np
import pytest
from tests import unit_inputs as U
from tests.test_gpu_units import BIT_SHARE_FLOOR, bits, rel_err, same, within_tolerance

pytestmark = pytest.mark.gpu
ALL = U.SURFACE_UNIT_SCENES + U.SURFACE_SCENES
RUNS = ("record", "record_plain", "sample", "eval")
SHAPE_NAMES = {3: "rectangle", 4: "disk", 5: "sphere", 6: "cylinder"}
UV_BOUND, FRAME_BOUND = 2e-6, 2e-5      # test_scene_ray_intersect_full_records' bound on its.uv, within_tolerance's bound on directions


@pytest.fixture(scope="module")
def surface_runs(mi, oracle, golden_scenes):
    """every scene through the oracle and the device, once: per scene the reference (inputs, oracle outputs, branches), the device's hits and its four runs"""
    out = {}; long_bit = oracle.Oracle.SURFACE_BRANCHES["ewa_long"]
    for name in ALL:
        r = U.surface_reference(oracle, golden_scenes, mi.scenes, name); inp = r["inp"]
        assert all(((r["runs"][run][1] & long_bit) == 0).all() for run in RUNS), name      # the census' cap on the EWA loops, checked again before any launch
        gs = mi.Scene(r["sc"]); hits, inst = gs.intersect(inp["rays"], with_instance=True)
        got = {"record": gs.surface_units("record", inp["rays"], hits, inst, inp["diff"]), "record_plain": gs.surface_units("record", inp["rays"], hits, inst),
               "sample": gs.surface_units("sample", inp["rays"], hits, inst, inp["diff"], r["query"]), "eval": gs.surface_units("eval", inp["rays"], hits, inst, None, r["wo_world"])}
        gs.close(); out[name] = dict(ref=r, hits=hits, inst=inst, got=got)
    return out


def record_within(got, ref):
    """a record that is not bit-equal still meets the project's bounds: the same hit, flags and record indices; non-finite exactly where the oracle is; uv within 2e-6;
    the frames and wi within 2e-5; tangents and the loaded texture values at err < 1e-4 (the bound of the filtered lookups).  The partials are printed, not bounded."""
    fin = np.isfinite(ref); ok = (np.isnan(got) == np.isnan(ref)).all(1) & (np.isinf(got) == np.isinf(ref)).all(1)
    g, r = np.where(fin, got, 0.0), np.where(fin, ref, 0.0)
    ok &= (bits(got[:, 37:42]) == bits(ref[:, 37:42])).all(1) & (got[:, 18:22] == ref[:, 18:22]).all(1)
    ok &= np.abs(g[:, 0:2] - r[:, 0:2]).max(1) <= UV_BOUND
    for a, b in ((25, 37), (42, 51)): ok &= np.abs(g[:, a:b] - r[:, a:b]).max(1) <= FRAME_BOUND
    for a, b in ((2, 5), (5, 8), (12, 15), (15, 18), (22, 25)): ok &= rel_err(g[:, a:b], r[:, a:b]) < 1e-4
    return ok


def classify(run):
    """per case: is it a hit (on both sides), the tangent source the oracle reports, the record at the head of its chain, its leaf record"""
    r = run["ref"]; sc = r["sc"]; rec, br = r["runs"]["record_plain"]
    return dict(hit=(br & (1 << 20)) == 0, source=(br & 7).astype(int), head=U.hit_records(sc, rec), leaf=rec[:, 21].astype(int))


def describe(name, mode, i, run, got, ref):
    inp = run["ref"]["inp"]
    return (f"{name} {mode} case {i} ({inp['kind'][i] or 'plain'}, differentials {inp['diff_kind'][i] or 'x%g' % inp['scale'][i]}): ray {inp['rays'][i].tolist()} hit {run['hits'][i].tolist()} "
            f"instance {int(run['inst'][i])}\n    device {got[i].tolist()}\n    oracle {ref[i].tolist()}")


def test_surface_units_hits_agree(surface_runs):
    """the chained intersection is the oracle's: (t, u, v, prim, instance) equal bit for bit, a miss on one side is a miss on the other"""
    for name, run in surface_runs.items():
        rec, br = run["ref"]["runs"]["record_plain"]; miss = (br & (1 << 20)) != 0
        dev = np.concatenate([run["hits"], run["inst"][:, None].astype(np.float32)], 1)
        eq = np.where(miss, run["hits"][:, 3] < 0, (bits(dev) == bits(rec[:, 37:42])).all(1))
        for i in np.flatnonzero(~eq)[:8]: print(f"[unit-surface] {name} case {i}: device hit {dev[i].tolist()} oracle {rec[i, 37:42].tolist()}")
        assert eq.all(), (name, float(eq.mean()))


@pytest.mark.parametrize("name", ALL)
def test_surface_units_triangles_without_libm(surface_runs, name):
    """triangle hits, instanced or not, whose chain and leaf call no math-library routine (unit_inputs.surface_no_libm): every output bit of every case of all four
    runs equals the oracle's (NaN counts as equal to NaN)"""
    run = surface_runs[name]; c = classify(run); sc = run["ref"]["sc"]; n = 0
    for mode in RUNS:
        exact = np.array([h >= 0 and U.surface_no_libm(sc, int(h), mode in ("record", "sample")) for h in c["head"]]) & c["hit"] & (c["source"] <= 2)
        got, ref = run["got"][mode][exact], run["ref"]["runs"][mode][0][exact]; eq = same(got, ref); n += len(eq)
        for i in np.flatnonzero(~eq)[:8]: print("[unit-surface] " + describe(name, mode, np.flatnonzero(exact)[i], run, run["got"][mode], run["ref"]["runs"][mode][0]))
        assert eq.all(), (name, mode, float(eq.mean()), int((~eq).sum()))
    assert n > 0 or name == "textured_shapes"
    miss = ~c["hit"]
    for mode in RUNS: assert (run["got"][mode][miss] == 0).all(), (name, mode)      # a miss writes zeros


def _pooled(surface_runs, select, key):
    pools = {}
    for name, run in surface_runs.items():
        c = classify(run); sc = run["ref"]["sc"]
        for mode in RUNS:
            pick = select(sc, c, mode); got, ref = run["got"][mode], run["ref"]["runs"][mode][0]
            eq = same(got, ref); tol = record_within(got, ref) if mode.startswith("record") else within_tolerance(got, ref, mode == "sample")
            for i in np.flatnonzero(pick & ~eq): print("[unit-surface] " + ("" if tol[i] else "OUT OF TOLERANCE ") + describe(name, mode, i, run, got, ref))
            for k in np.unique(key(sc, c)[pick]):
                sel = pick & (key(sc, c) == k); p = pools.setdefault(str(k), dict(n=0, eq=0, bad=0)); p["n"] += int(sel.sum()); p["eq"] += int((sel & eq).sum()); p["bad"] += int((sel & ~eq & ~tol).sum())
    return pools


def test_surface_units_triangles_with_libm(surface_runs):
    """every other triangle hit, pooled per leaf type over all scenes and runs: at least 0.9999 of the cases equal the oracle in every output bit; every case outside that
    share is printed and still meets the project's tolerances (within_tolerance on the query outputs, record_within on the record)"""
    def select(sc, c, mode):
        exact = np.array([h >= 0 and U.surface_no_libm(sc, int(h), mode in ("record", "sample")) for h in c["head"]])
        return c["hit"] & (c["source"] <= 2) & ~exact
    key = lambda sc, c: np.array([U.TYPE_NAMES[sc.bsdfs[l]["type"]] for l in c["leaf"]], dtype=object)
    pools = _pooled(surface_runs, select, key); assert pools
    for t, p in sorted(pools.items()): print(f"[bit-share] surface {t}: {p['eq'] / p['n']:.6f} of {p['n']} cases, {p['n'] - p['eq']} outside, {p['bad']} outside the tolerances")
    for t, p in pools.items(): assert p["bad"] == 0 and p["eq"] / p["n"] >= BIT_SHARE_FLOOR, (t, p)


def test_surface_units_analytic_shapes(surface_runs):
    """hits on analytic shapes (their parameterisations call atan2 / acos / sin), pooled per shape kind: bit share >= 0.9999; a case outside it has uv within 2e-6 and
    frames within 2e-5, and is finite where the oracle is (record_within / within_tolerance); its texture values and partials are printed"""
    select = lambda sc, c, mode: c["hit"] & (c["source"] >= 3)
    key = lambda sc, c: np.array([SHAPE_NAMES.get(s, "triangle") for s in c["source"]], dtype=object)
    pools = _pooled(surface_runs, select, key); assert set(pools) == set(SHAPE_NAMES.values())
    for t, p in sorted(pools.items()): print(f"[bit-share] surface {t}: {p['eq'] / p['n']:.6f} of {p['n']} cases, {p['n'] - p['eq']} outside, {p['bad']} outside the tolerances")
    for t, p in pools.items(): assert p["bad"] == 0 and p["eq"] / p["n"] >= BIT_SHARE_FLOOR, (t, p)


def _normalize(v):
    inv = np.float32(1) / np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2]); return v * inv[:, None]


def _dot(a, b):
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


def test_surface_units_frames_without_oracle(surface_runs):
    """properties of the perturbed frame that need no oracle, on the device's own mode-0 outputs of the unit scene: with bump scale 0 the perturbed normal is the shading
    normal up to the documented flip to the geometric side; under the (0.5, 0.5, 1) normal map it IS the shading normal, bit for bit; and the tangent of a normal-mapped
    frame is normalize(dpdu - n (n . dpdu)), bit for bit when recomputed in float32 from the record's dpdu and n"""
    run = surface_runs["surface_units_edges"]; sc = run["ref"]["sc"]; c = classify(run); seen = set()
    for mode in ("record", "record_plain"):
        rec = run["got"][mode]; ns, dpdu, ps, pn = rec[:, 42:45], rec[:, 2:5], rec[:, 25:28], rec[:, 31:34]
        for m in np.unique(c["head"][c["head"] >= 0]):
            b = sc.bsdfs[m]; at = (c["head"] == m) & c["hit"] & np.isfinite(rec).all(1)
            if b["type"] == 11 and b["alpha"] == 0.0:
                assert at.sum() > 50 and (np.minimum(np.abs(pn[at] - ns[at]).max(1), np.abs(pn[at] + ns[at]).max(1)) <= FRAME_BOUND).all(); seen.add("scale 0")
            if b["type"] == 12 and sc.textures[b["texture"]]["color0"] == U.CONSTANT_NORMALS[0]:
                assert at.sum() > 50 and (bits(pn[at]) == bits(ns[at])).all(); seen.add("unperturbed")
            if b["type"] == 12 and at.any():
                n, d = pn[at], dpdu[at]; want = _normalize(d - n * _dot(n, d)[:, None]); ok = np.isfinite(want).all(1)
                assert (bits(ps[at][ok]) == bits(want[ok])).all(), (int(m), mode); seen.add("tangent")
    assert seen == {"scale 0", "unperturbed", "tangent"}
