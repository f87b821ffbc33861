"""CPU: the shape rule of the path pools (mi_debug_pool_shape, a pure host function) against its plain-Python restatement, the rows tests/test_gpu_pool_geometry.py runs
on the GPU against the purpose each is there for, and the emitter / light-triangle tables of that file's three-emitter scene -- so that the GPU tests cannot drift
into testing nothing."""
import numpy as np
import pytest
from tests import test_gpu_pool_geometry as G

PATHS = [1, 63, 64, 65, 6000, 65472, 65473, 2 ** 20 + 1, 2 ** 28]
SEGMENTS = [None, 0, 1, 7, 10 ** 6]


@pytest.mark.parametrize("integrator", [0, 1, 2])
@pytest.mark.parametrize("has_rc", [False, True])
def test_restated_rule_equals_the_library(mi, integrator, has_rc):
    refused = 0
    for paths in PATHS + [2 ** 24, 2 ** 26 + 5, 2 ** 28 - 64, 2 ** 28 - 63]:
        for seg in SEGMENTS:
            for grids in ({}, dict(grid_extend=1, grid_shade=1, grid_shadow=1), dict(grid_extend=0, grid_shade=600, grid_shadow=10 ** 5)):
                want = G.pool_rule(paths, has_rc, integrator, seg, **grids)
                if want is None:
                    with pytest.raises(mi.MiError) as e:
                        mi.api.pool_shape(paths, has_rc, integrator, seg or 0, **grids)
                    assert e.value.code == 1 and "2^28" in str(e.value); refused += 1
                    continue
                got = mi.api.pool_shape(paths, has_rc, integrator, seg or 0, **grids)
                assert got == want, (paths, seg, grids, got, want)
                n_seg, cap = got["n_seg"], got["cap"]
                assert n_seg >= 1 and cap % 64 == 0 and cap >= 64 and n_seg * cap >= paths and n_seg * cap < 2 ** 28
                assert n_seg <= max(1, -(-paths // 64))                                    # the ceil(paths / 64) clamp
                assert (n_seg - 1) * cap < paths + 64 * n_seg                              # rounding up to 64 is all the slack there is
                if integrator != 0: assert cap <= 65472                                    # the volumetric re-grid
                if seg in (None, 0): assert got == mi.api.pool_shape(paths, has_rc, integrator, 0, **grids) == G.pool_rule(paths, has_rc, integrator, None, **grids)      # 0 -> unset
    assert refused >= len(SEGMENTS) * 3 * 2      # 2^28 paths (and 2^28 - 63, which rounds up to it) are refused whatever the overrides say
    assert G.pool_rule(2 ** 28, has_rc, integrator) is None and G.pool_rule(2 ** 27, has_rc, integrator) is not None


def test_shape_rule_landmarks(mi):
    """the numbers the issue and DESIGN.md quote"""
    P = mi.api.pool_shape
    assert (P(6000)["n_seg"], P(6000)["cap"]) == (94, 64) and P(6000)["grid_shade"] == 94
    assert all(P(p)["cap"] == 64 for p in (1, 64, 65, 6000, 82944, 147456, 2 ** 20))                   # under 1 M paths: one chunk per segment
    assert P(2 ** 20 + 1)["cap"] == 128
    assert (P(64 << 20)["n_seg"], P(64 << 20)["cap"]) == (16384, 4096) and P(64 << 20)["grid_shade"] == 768      # production: 64 M paths per pool
    assert (P(64 << 20, True)["n_seg"], P(64 << 20, True)["cap"]) == (65536, 1024) and P(64 << 20, True)["grid_shade"] == 512
    assert (P(65472, False, 1, 1)["n_seg"], P(65472, False, 1, 1)["cap"]) == (1, 65472)
    assert (P(65473, False, 2, 1)["n_seg"], P(65473, False, 2, 1)["cap"]) == (2, 32768)
    assert (P(65473, False, 0, 1)["n_seg"], P(65473, False, 0, 1)["cap"]) == (1, 65536)               # the path integrator has no such limit


def test_gpu_rows_have_the_shape_they_are_there_for():
    want = {None: (94, 64, 1, 48), 47: (47, 128, 2, 112), 6: (6, 1024, 16, 880), 3: (3, 2048, 32, 1904), 1: (1, 6016, 94, 6000)}      # n_seg, cap, chunks per segment, last segment
    assert [s for s, _ in G.SEGMENT_ROWS] == list(want)
    for seg, expect in G.SEGMENT_ROWS:
        for has_rc in (False, True):
            for integrator in (0, 1, 2):
                r = G.pool_rule(G.N_PAIRS, has_rc, integrator, seg); assert (r["n_seg"], r["cap"]) == expect
        n_seg, cap, chunks, tail = want[seg]; occ = G.occupancy(G.N_PAIRS, n_seg, cap)
        assert expect == (n_seg, cap) and cap // 64 == chunks and occ[-1] == tail and sum(occ) == G.N_PAIRS and all(o == cap for o in occ[:-1])
        if seg not in (None, 1): assert tail % 64 != 0 or tail < cap                       # a part-filled last chunk or a short last segment
    assert 112 % 64 == 48 and 880 % 64 == 48 and 1904 % 64 == 48 and 6000 % 64 == 48      # every forced shape ends in a chunk of 48 paths
    for paths, seg, expect in G.BIG_ROWS:
        for has_rc in (False, True):
            r = G.pool_rule(paths, has_rc, 0, seg); assert (r["n_seg"], r["cap"]) == expect
    assert G.BIG_ROWS[0][2][1] > 8192 and G.BIG_ROWS[0][2][1] <= 0xFFFF and G.BIG_ROWS[1][2][1] > 0xFFFF
    assert G.pool_rule(70000, False, 1, 1)["n_seg"] == 2                                   # (the volumetric integrators would re-grid that one)
    paths, seg, expect = G.SORTED_ROW; r = G.pool_rule(paths, True, 0, seg)
    assert (r["n_seg"], r["cap"]) == expect == (2, 4096) and 16 + 8 * 4096 + 16 <= 64 * 1024 and G.occupancy(paths, 2, 4096) == [4096, 4004]
    r = G.pool_rule(G.N_PAIRS, True, 0, 4); assert (r["n_seg"], r["cap"]) == (4, 1536) and G.occupancy(G.N_PAIRS, 4, 1536)[-1] == 1392      # test_sorted_shading_at_cap_1536
    assert set(G.SORT_STATE["veach_small"]) == {e[1] for _, e in G.SEGMENT_ROWS} | {1536}
    for name, table, limit in (("veach_small", 52156, 1670), ("cbox_materials", 31388, 4266), ("instanced_garden", 36044, 3684)):      # the written-out states = the size rule
        assert name in G.SCENES and set(G.SORT_STATE[name]) >= {e[1] for _, e in G.SEGMENT_ROWS}
        for cap, state in G.SORT_STATE[name].items():
            info = dict(has_roughconductor=1, integrator=0, cap=cap, shade_table_bytes=table); assert G.sort_rule(info) == state == (1 if cap <= limit else 0), (name, cap)
        assert 0 in G.SORT_STATE[name].values() and 1 in [v for c, v in G.SORT_STATE[name].items() if c > 64]      # both modes are met at more than one chunk
    for integrator in (1, 2):
        a = G.pool_rule(G.VOL_EDGE, False, integrator, 1); b = G.pool_rule(G.VOL_EDGE + 1, False, integrator, 1)
        assert (a["n_seg"], a["cap"]) == (1, 65472) and a["cap"] // 64 == 1023 and (b["n_seg"], b["cap"]) == (2, 32768)
    # the anchor of every case: one chunk per segment
    for paths in (100, 6000, 8100, 20000, 70000, 65472, 65473):
        r = G.pool_rule(paths); assert (r["n_seg"], r["cap"]) == (-(-paths // 64), 64)
    # films of (c) / (d): 5 and 40 segments give segments of several chunks at the batch sizes those tests reach
    for npix in (96 * 54, 96 * 96):
        for planes in (1, 2, 3, 4, 7):
            assert G.pool_rule(npix * planes, segments=5)["cap"] >= 1088
        assert G.pool_rule(npix * 2, segments=40)["cap"] >= 320
    assert G.pool_rule(37 * 23, segments=3)["cap"] == 320


def test_three_emitter_scene_has_both_empty_bins(mi, oracle):
    """tri_lights: emitter table (0, 1/2, 1/2, 1) and light-triangle table (0, 1/2, 1/2, 1), each with its zero-width bin at index 1 -- and, on the oracle alone, the
    first emitter-sampling draw of the 6000 pairs lands next to those bins from both sides (within 2^-9 of 1/2: the whole-table search counts entries below x, so the
    samples that tell its tie rules from the binary search's are the ones around the repeated entry), and on every bin that is not empty."""
    S = mi.scenes; sc = G.tri_lights(S)
    assert [e["type"] for e in sc.emitters] == [S.EMITTER_POINT, S.EMITTER_SPOT, S.EMITTER_AREA] and [e["weight"] for e in sc.emitters] == [1.0, 0.0, 1.0]
    w = np.array([e["weight"] for e in sc.emitters]); cdf = np.concatenate([[0], np.cumsum(w) / w.sum()])
    assert cdf.tolist() == [0, 0.5, 0.5, 1.0]
    light = [s for s in sc.shapes if s["emitter"] >= 0]; assert len(light) == 1 and light[0]["emitter"] == 2 and light[0]["tri_count"] == 3
    tri = sc.pos[sc.idx[light[0]["first_tri"]:light[0]["first_tri"] + 3]].astype(np.float32)
    area = np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1) * np.float32(0.5)      # float32 throughout: exactly zero, not merely small
    assert area.dtype == np.float32 and area.tolist() == [0.5, 0.0, 0.5]
    assert len(sc.emitters) <= 3 and light[0]["tri_count"] <= 3                            # both tables qualify for the whole-table search
    pairs = G.make_pairs(sc, G.N_PAIRS); out = oracle.Oracle(sc).render_samples(pairs, log=True)
    assert np.isfinite(out["li"]).all() and (out["li"] >= 0).all() and out["li"].max() > 0
    hit = out["nvals"] >= 4; sx, sy = out["vals"][hit, 2], out["vals"][hit, 3]           # draws 0, 1: the film position; 2, 3: emitter sampling at the camera hit
    assert hit.mean() > 0.5
    eps = 2.0 ** -9
    for name, x in (("emitter table", sx), ("light-triangle table", sy)):
        below = int(((x <= 0.5) & (x > 0.5 - eps)).sum()); above = int(((x > 0.5) & (x < 0.5 + eps)).sum())
        print(f"[pool-geometry] tri_lights {name}: {below} draws within 2^-9 below 1/2, {above} above, {int((x == 0.5).sum())} exactly on it")
        assert below >= 3 and above >= 3, (name, below, above)
        assert (x < 0.25).any() and (x > 0.75).any()
    # the area light was drawn (sx > 1/2) with sy on either side of its empty bin
    assert ((sx > 0.5) & (sy < 0.5)).sum() > 100 and ((sx > 0.5) & (sy > 0.5)).sum() > 100


def test_first_empty_variant_reaches_the_empty_bin_rules(mi, oracle):
    """tri_lights(first_empty=True): emitter table (0, 0, 0, 1), light-triangle table (0, 0, 1/2, 1); pair 0 -- pixel (0, 0), sample 0, the Sobol point of index 0 -- draws
    exactly 0 for the emitter and for the triangle at its camera hit: DiscreteDistribution::sample answers 0 with the first bin and has to step over the empty ones"""
    S = mi.scenes; sc = G.tri_lights(S, first_empty=True)
    assert [e["weight"] for e in sc.emitters] == [0.0, 0.0, 1.0] and sc.emitters[2]["type"] == S.EMITTER_AREA and sc.sampler == S.SAMPLER_SOBOL and sc.seed == 0
    light = [s for s in sc.shapes if s["emitter"] >= 0][0]; tri = sc.pos[sc.idx[light["first_tri"]:light["first_tri"] + 3]].astype(np.float32)
    area = np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1) * np.float32(0.5)
    assert area.tolist() == [0.0, 0.5, 0.5]
    pairs = G.make_pairs(sc, G.N_PAIRS); assert pairs[0].tolist() == [0, 0, 0]
    out = oracle.Oracle(sc).render_samples(pairs, log=True)
    assert np.isfinite(out["li"]).all() and out["li"].max() > 0
    assert out["nvals"][0] >= 4 and (out["vals"][0, :4] == 0).all()                      # the camera ray of pair 0 hits the room and both emitter-sampling draws are 0
    assert out["li"][0].max() > 0                                                         # ... and the sample it then takes from the area light arrives
