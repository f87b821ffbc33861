"""CPU: the census of the surface-step inputs (tests/unit_inputs.py, surface_inputs) through the oracle alone (orc_surface_units).  It gates what
tests/test_gpu_surface_units.py may claim: every branch the oracle reports is taken by at least 1 % of the cases of the pool it belongs to, few rays miss, and the oracle's
non-finite outputs have the causes the generator planted and no others."""
import numpy as np
import pytest
from tests import unit_inputs as U

ALL = U.SURFACE_UNIT_SCENES + U.SURFACE_SCENES
LAYERED = ["layered_room", "layered_room_procedural"]
UNITS = U.SURFACE_UNIT_SCENES
FLOOR = 0.01
# branch -> the scenes whose cases form its pool (the scenes that hold what the branch needs)
TANGENT_POOLS = {"uv_tangents": LAYERED + ["masked_room", "bitmap_room", "textured_plastics", "textured_plastics_smooth"] + UNITS, "edges": ["masked_room", "textured_shapes"] + UNITS,
                 "rectangle": ["textured_shapes"], "disk": ["textured_shapes"], "sphere": ["textured_shapes", "surface_units_edges"], "cylinder": ["textured_shapes"]}
FLAG_POOLS = {"instanced": ["surface_units_instanced"], "degenerate_uv": ["surface_units_edges"],
              "texture_only": ["bitmap_room", "textured_plastics", "textured_plastics_smooth", "textured_shapes"] + UNITS, "mask": LAYERED + ["masked_room", "textured_shapes", "surface_units_instanced"],
              "mask_bump": LAYERED + ["surface_units_instanced"], "bump_bitmap": ["layered_room"] + UNITS, "bump_procedural": LAYERED, "normalmap": LAYERED + UNITS, "bump_mixture": LAYERED,
              "coat_textured": ["surface_units_edges"], "ewa": ["bitmap_room", "textured_shapes"] + UNITS, "filter_fallback": ["bitmap_room", "textured_shapes"] + UNITS,
              "bump_flipped": LAYERED + UNITS, "sign_change": LAYERED + UNITS}
PARTIALS_POOLS = {"prx_or_pry_zero": ALL, "regular": ALL}
# "solve_failed" needs parallel tangents in the projection plane: UV tangents come out of an inverted 2 x 2 system or out of coordinateSystem, edge vectors of a triangle
# that can be hit are independent, and of the analytic shapes only the sphere has a point where one tangent vanishes (dpdu = 0 at its poles).  Its pool is the sphere hits of
# the unit scene, whose sphere is axis-aligned so that a ray along the axis meets the pole exactly.
# "zero_tangents" (dpdu and dpdv both zero) cannot be reached through the scene front end: computeUVTangents leaves both zero only for a triangle of zero area, which no ray
# hits, and no analytic parameterisation has a point where both vanish (at a sphere's pole dpdv = (0, z, 0) pi).  The branch stays covered by reading alone.
UNREACHABLE = {"zero_tangents"}


@pytest.fixture(scope="module")
def refs(mi, oracle, golden_scenes):
    return {name: U.surface_reference(oracle, golden_scenes, mi.scenes, name) for name in ALL}


def _pool(refs, scenes, run="record"):
    return np.concatenate([refs[s]["runs"][run][1] for s in scenes])


def test_surface_census_branches(refs, oracle):
    O = oracle.Oracle; shares = {}
    for k, scenes in TANGENT_POOLS.items(): shares["tangent " + k] = float(np.mean((_pool(refs, scenes) & 7) == O.SURFACE_TANGENTS[k]))
    for k, scenes in PARTIALS_POOLS.items(): shares["partials " + k] = float(np.mean(((_pool(refs, scenes) >> 13) & 7) == O.SURFACE_PARTIALS[k]))
    for k, scenes in FLAG_POOLS.items():
        runs = ("record", "sample", "eval") if k == "sign_change" else ("record",)      # the sign change of wi (record), of the sampled and of the supplied direction
        for run in runs: shares[f"{k} ({run})"] = float(np.mean((_pool(refs, scenes, run) & O.SURFACE_BRANCHES[k]) != 0))
    br = refs["surface_units_edges"]["runs"]["record"][1]; sphere = (br & 7) == O.SURFACE_TANGENTS["sphere"]
    shares["partials solve_failed (sphere hits)"] = float(np.mean(((br[sphere] >> 13) & 7) == O.SURFACE_PARTIALS["solve_failed"]))
    for k, v in sorted(shares.items()): print(f"[census] surface {k}: {v:.4f}")
    low = {k: v for k, v in shares.items() if v < FLOOR}
    assert not low, low
    assert set(O.SURFACE_PARTIALS) - {"none"} == {k for k in PARTIALS_POOLS} | {"solve_failed"} | UNREACHABLE
    # later bounces: no partials at all, and no filtered lookup
    for name, r in refs.items():
        plain = r["runs"]["record_plain"][1]; hit = (plain & O.SURFACE_BRANCHES["miss"]) == 0
        assert (((plain[hit] >> 13) & 7) == 0).all() and ((plain & (O.SURFACE_BRANCHES["ewa"] | O.SURFACE_BRANCHES["filter_fallback"])) == 0).all(), name
    # the EWA loops stay short on every case: nothing has to be kept from the device
    assert all(((r["runs"][run][1] & O.SURFACE_BRANCHES["ewa_long"]) == 0).all() for r in refs.values() for run in ("record", "sample"))


@pytest.mark.parametrize("name", ALL)
def test_surface_census_misses_and_non_finite(refs, oracle, name):
    """at most 5 % misses; at most 10 % non-finite oracle outputs, all of them from a planted cause: a non-finite differential (runs with differentials), the
    (0.5, 0.5, 0.5) normal map (the perturbed normal is normalize(0)), the pole of a sphere (dpdu = 0: the shading tangent is normalize(0))"""
    r = refs[name]; sc = r["sc"]; inp = r["inp"]; O = oracle.Oracle; rec = r["runs"]["record_plain"][0]
    head = U.hit_records(sc, rec); zero_normal = np.isin(head, sorted(U.zero_normal_records(sc)))
    pole = ((r["runs"]["record_plain"][1] & 7) == O.SURFACE_TANGENTS["sphere"]) & (rec[:, 2:5] == 0).all(1)
    for run, (out, br) in r["runs"].items():
        miss = (br & O.SURFACE_BRANCHES["miss"]) != 0; nf = ~np.isfinite(out).all(1)
        assert miss.mean() <= 0.05 and (out[miss] == 0).all(), (run, float(miss.mean()))
        planted = zero_normal | pole | ((inp["diff_kind"] == "nonfinite") if run in ("record", "sample") else False)
        print(f"[census] surface {name} {run}: misses {miss.mean():.4f}, non-finite {nf.mean():.4f} (zero normal {int((nf & zero_normal).sum())}, pole {int((nf & pole).sum())})")
        assert nf.mean() <= 0.10 and not (nf & ~planted).any(), (run, float(nf.mean()), np.flatnonzero(nf & ~planted)[:8])
    assert (inp["diff_kind"] == "nonfinite").mean() > 0.04 and (inp["diff_kind"] == "perpendicular").mean() > 0.04 and (inp["kind"] == "graze").mean() > 0.15 and (inp["kind"] == "edge").mean() > 0.08
    assert {float(s) for s in np.unique(inp["scale"])} == set(U.DIFF_SCALES)


def test_surface_unit_scene_records(refs, oracle):
    """what the two unit scenes were built for is there and is hit: the instances' members behind every kind of record, bump scales 0, -1 and 1e4, the nearest-filter
    displacement, the three constant normal maps, the degenerate-UV triangle, the mesh without texture coordinates under a plain record"""
    O = oracle.Oracle
    r = refs["surface_units_instanced"]; rec, br = r["runs"]["record"]; inst = (br & O.SURFACE_BRANCHES["instanced"]) != 0
    assert set(np.unique(rec[inst, 41]).astype(int)) == {0, 1, 2}
    for k in ("texture_only", "bump_bitmap", "normalmap", "mask_bump"): assert ((br[inst] & O.SURFACE_BRANCHES[k]) != 0).mean() >= 0.05, k
    r = refs["surface_units_edges"]; sc = r["sc"]; rec, br = r["runs"]["record"]; head = U.hit_records(sc, rec)
    scales = {float(sc.bsdfs[m]["alpha"]) for m in np.unique(head[head >= 0]) if sc.bsdfs[m]["type"] == 11}; assert set(U.BUMP_SCALES) <= scales
    nearest = [m for m in range(len(sc.bsdfs)) if sc.bsdfs[m]["type"] == 11 and sc.textures[sc.bsdfs[m]["texture"]]["filter"] == 0]
    assert nearest and np.isin(head, nearest).mean() >= FLOOR and (rec[np.isin(head, nearest), 19] == 1).all()
    for i in range(3):
        m = [k for k in range(len(sc.bsdfs)) if sc.bsdfs[k]["type"] == 12 and sc.bsdfs[k]["texture"] == 3 + i]; assert np.isin(head, m).mean() >= FLOOR, i
    plain_no_uv = ((br & 7) == O.SURFACE_TANGENTS["edges"]) & ((br & (O.SURFACE_BRANCHES["texture_only"] | O.SURFACE_BRANCHES["bump_bitmap"] | O.SURFACE_BRANCHES["normalmap"])) == 0)
    assert plain_no_uv.mean() >= 0.05
