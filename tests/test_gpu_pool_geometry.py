"""GPU (MI355X): the wavefront stages at path-pool shapes of more than one 64-slot chunk per segment, and both settings of every switch that picks other code for the
same scene, against the oracle.

A pool of P paths is cut into n_seg segments of cap slots (mi_debug_pool_shape); the shade stages give a segment to one wave, which walks it in chunks of 64 and
carries its output offsets (survivors, shadow records, the class-sorted order list, the back-filled search / alpha records of the volumetric stages) from chunk to
chunk.  Below 1 M paths the default rule gives cap = 64 -- one chunk -- so every other oracle comparison of the suite runs that loop once.  Here MI355PT_SEGMENTS /
MI355PT_GRID_* (read when the pool is allocated), MI355PT_STREAMS (when the render is created) and MI355PT_NO_LDS_TABLES / MI355PT_SEARCH / MI355PT_BVH2 /
MI355PT_NO_PACKET (when the scene is committed) force the other shapes; every case asserts through Render.pool_info() that it ran at the shape it means, computed
by the plain-Python restatement of the rule below (tests/test_pool_geometry.py checks that restatement against the library and the rows against their purpose).

Two assertions per (scene, shape): the oracle, by the criterion of the scene's own test in tests/test_gpu_parity.py; and bit equality with the anchor shape (the
default one) for ALL pairs -- a path's additions to its accumulator happen in launch order by depth whichever slot it sits in, so the shape cannot move a bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KNOBS = ("MI355PT_SEGMENTS", "MI355PT_GRID_EXTEND", "MI355PT_GRID_SHADE", "MI355PT_GRID_SHADOW", "MI355PT_STREAMS", "MI355PT_NO_LDS_TABLES", "MI355PT_SEARCH",
         "MI355PT_BVH2", "MI355PT_NO_PACKET")


# ---------------------------------------------------------------------------------------------- the rule, restated
def pool_rule(paths, has_rc=False, integrator=0, segments=None, grid_extend=None, grid_shade=None, grid_shadow=None):
    """(n_seg, cap, grid_extend, grid_shade, grid_shadow) of a pool of `paths` paths, or None where the library refuses (2^28 slots or more).  None / 0 = unset."""
    n_seg = segments or (min(max(16384, paths // 1024), 1 << 18) if has_rc else 16384)
    n_seg = min(n_seg, max(-(-paths // 64), 1))                                  # never more segments than 64-path chunks
    if integrator != 0 and -(-paths // n_seg) > 65472: n_seg = -(-paths // 65472)      # volumetric: two 16-bit record counts per segment
    cap = -(-(-(-paths // n_seg)) // 64) * 64
    if cap * n_seg >= 1 << 28: return None
    return dict(n_seg=n_seg, cap=cap, grid_extend=min(n_seg, grid_extend or 4096), grid_shade=min(n_seg, grid_shade or (512 if has_rc else 768)),
                grid_shadow=min(n_seg, grid_shadow or 4096))


def occupancy(paths, n_seg, cap):
    """paths per segment as k_generate lays them: segment s holds the paths s * cap .. (s + 1) * cap - 1"""
    return [min(cap, max(0, paths - s * cap)) for s in range(n_seg)]


N_PAIRS = 6000
# (a) MI355PT_SEGMENTS -> the shape 6000 paths get and what it is there for (tests/test_pool_geometry.py asserts both columns)
SEGMENT_ROWS = [(None, (94, 64)),      # today's shape: the anchor
                (47, (47, 128)),       # two chunks; the last segment holds 112 paths: a ragged second chunk
                (6, (6, 1024)),        # production size of rough-conductor scenes: 16 chunks, 880 paths in the last segment
                (3, (3, 2048)),        # 1904 paths in the last segment
                (1, (1, 6016))]        # the whole batch in ONE wave of the shade stage; every other wave and workgroup finds no segment
BIG_ROWS = [(20000, 2, (2, 10048)),    # cap > 8192: the order list does not fit, unsorted shading
            (70000, 1, (1, 70016))]    # cap > 0xFFFF: path integrator only
SORTED_ROW = (8100, 2, (2, 4096))      # independent sampler (16 B of tables): the 32 KB order list of cap = 4096 fits, the shade stage sorts; 4004 paths in the last segment
VOL_EDGE = 65472                        # slots per segment the volumetric stages may reach (1023 chunks): 65472 paths in ONE segment, 65473 re-grid to two

# scene -> environment at commit time; criterion of its test in test_gpu_parity.py ("bits": every pair bit-equal; "libm": bit_share > 0.9999 + the err shares)
SCENES = {"cornell_small": ({}, "bits"),
          "veach_small": ({}, "libm_veach"),
          "cbox_materials": ({}, "bits"),
          "atrium_small": ({"MI355PT_BVH2": "0", "MI355PT_NO_PACKET": "1"}, "libm_atrium"),
          "instanced_garden": ({}, "bits"),
          "fog_box": ({}, "bits"),
          "fog_mis": ({}, "bits")}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def make_pairs(sc, n, seed=2025):
    """n random (pixel, sample) triples, the four corners first (as test_full_size_configs_spot_check_vs_oracle draws them)"""
    rng = np.random.default_rng(seed)
    pairs = np.stack([rng.integers(0, sc.width, n), rng.integers(0, sc.height, n), rng.integers(0, sc.spp, n)], 1).astype(np.uint32)
    pairs[:4] = [[0, 0, 0], [sc.width - 1, sc.height - 1, sc.spp - 1], [sc.width - 1, 0, sc.spp // 2], [0, sc.height - 1, 1]]
    return pairs


def tri_lights(S, width=64, height=64, spp=16, sampler=None, seed=0, first_empty=False):
    """A room with exactly three emitters -- point (weight 1), spot (weight 0), area (weight 1): emitter table (0, 1/2, 1/2, 1), a zero-width bin at index 1 -- whose
    area light is ONE mesh of three triangles, the middle one degenerate (its third vertex is the midpoint of the other two): area table (0, 1/2, 1/2, 1) as well.
    Both tables are short enough for cdfSampleReuse's whole-table search (MI355PT_SEARCH bits 0 and 1).  A bin in the MIDDLE of a table is never the search's first
    answer (the number of entries below x cannot stop between two equal entries), so this variant runs the search around a repeated entry but does NOT reach the
    rules that step over an empty bin.  first_empty = True does: point and spot both have weight 0 -- emitter table (0, 0, 0, 1) -- and the degenerate triangle comes
    first -- area table (0, 0, 1/2, 1); the Sobol point of index 0 (pixel (0, 0), sample 0: every draw exactly 0) then lands on the empty first bin of both tables
    and has to be moved on twice in the first and once in the second."""
    b = S._Builder()
    white = b.bsdf(reflectance=(0.7, 0.7, 0.7)); red = b.bsdf(reflectance=(0.6, 0.1, 0.1)); blue = b.bsdf(reflectance=(0.1, 0.2, 0.6)); lm = b.bsdf(reflectance=(0.5, 0.5, 0.5))
    b.begin(); b.quad([(4, 0, 0), (0, 0, 0), (0, 0, 4), (4, 0, 4)]); b.end(white)              # floor
    b.begin(); b.quad([(4, 4, 0), (4, 4, 4), (0, 4, 4), (0, 4, 0)]); b.end(white)              # ceiling
    b.begin(); b.quad([(4, 0, 4), (0, 0, 4), (0, 4, 4), (4, 4, 4)]); b.end(white)              # back
    b.begin(); b.quad([(0, 0, 4), (0, 0, 0), (0, 4, 0), (0, 4, 4)]); b.end(blue)               # x = 0
    b.begin(); b.quad([(4, 0, 0), (4, 0, 4), (4, 4, 4), (4, 4, 0)]); b.end(red)                # x = 4
    b.begin()                                                                                  # the light: (v0 v1 v2), (v0 mid v2) -- zero area --, (v0 v2 v3)
    base = len(b.verts); b.verts.extend([(2.5, 3.9, 1.5), (2.5, 3.9, 2.5), (1.5, 3.9, 2.5), (1.5, 3.9, 1.5), (2.0, 3.9, 2.0)])
    good, flat = [(base, base + 1, base + 2), (base, base + 2, base + 3)], (base, base + 4, base + 2)
    b.tris.extend([flat] + good if first_empty else [good[0], flat, good[1]])
    b.end(lm, radiance=(12.0, 10.0, 6.0))
    b.begin()                                                                                  # a block, so that shadow rays find something
    b.quad([(1, 1, 1.5), (1, 1, 2.5), (2, 1, 2.5), (2, 1, 1.5)]); b.quad([(2, 0, 1.5), (2, 1, 1.5), (2, 1, 2.5), (2, 0, 2.5)])
    b.quad([(1, 0, 1.5), (1, 1, 1.5), (2, 1, 1.5), (2, 0, 1.5)]); b.quad([(1, 0, 2.5), (1, 1, 2.5), (1, 1, 1.5), (1, 0, 1.5)])
    b.quad([(2, 0, 2.5), (2, 1, 2.5), (1, 1, 2.5), (1, 0, 2.5)]); b.end(white)
    cam = S.look_at((2, 2, -5.0), (2, 2, -4.0), (0, -1, 0))     # the corner rays of the film still enter the room; up is down, so that pixel (0, 0) sees the floor, which the light reaches
    sc = S.finish_scene(b.verts, b.tris, b.shapes, b.bsdfs, b.emitters, cam, 40.0, 0.1, 100.0, width, height, spp, S.SAMPLER_SOBOL if sampler is None else sampler, 6, 4,
                        seed=seed, name="tri_lights")
    return S.add_scene_emitters(sc, [S.point_emitter((1.0, 3.0, 1.0), (6.0, 8.0, 12.0), weight=0.0 if first_empty else 1.0),
                                     S.spot_emitter((3.5, 3.5, 0.5), (2.0, 0.0, 2.5), (40.0, 30.0, 20.0), cutoff=30.0, beam=20.0, weight=0.0)])


# ---------------------------------------------------------------------------------------------- shared state
_cases = {}


def clear_knobs(monkeypatch):
    for k in KNOBS: monkeypatch.delenv(k, raising=False)


def scene_of(mi, golden_scenes, name):
    return tri_lights(mi.scenes, first_empty=name.endswith("first_empty")) if name.startswith("tri_lights") else golden_scenes[name]


def check_shape(r, paths, segments=None, expect=None, **grids):
    """the render ran in the shape the restated rule gives for its own inputs (and, where the caller names one, in THAT shape); returns pool_info()"""
    info = r.pool_info(); want = pool_rule(paths, info["has_roughconductor"], info["integrator"], segments, **grids)
    assert want is not None and {k: info[k] for k in want} == want, (info, want)
    if expect is not None: assert (info["n_seg"], info["cap"]) == tuple(expect), (info, expect)
    assert info["pool_paths"] == paths
    assert info["sorted"] == sort_rule(info), info
    return info


def sort_rule(info):
    """whether the shade stage of this render reads its segments through the class-sorted order list (mi_launch_shade): a scene with rough conductors under the path
    integrator, cap <= 8192, and the launch's LDS in front of the list (shade_table_bytes: Sobol tables + scene tables, as the library reports them) rounded up to
    16 B + four order lists of cap 16-bit entries + 16 B within 64 KB"""
    if not info["has_roughconductor"] or info["integrator"] != 0 or info["cap"] > 8192: return 0
    return 1 if -(-info["shade_table_bytes"] // 16) * 16 + 8 * info["cap"] + 16 <= 64 * 1024 else 0


# cap -> sort state of the scenes with rough conductors, written out so that no row can slip into the other mode unnoticed (sort_rule must agree with it).  The LDS in
# front of the order list (Sobol tables + scene tables, shade_table_bytes) is 52156 B on veach_small (32768 B of them Sobol tables: maxDepth 12), 31388 B on
# cbox_materials and 36044 B on instanced_garden; 8 B x cap + 16 B have to fit behind it within 64 KB: cap <= 1670, 4266 and 3684
SORT_STATE = {"veach_small": {64: 1, 128: 1, 1024: 1, 1536: 1, 2048: 0, 6016: 0},
              "cbox_materials": {64: 1, 128: 1, 1024: 1, 2048: 1, 6016: 0},
              "instanced_garden": {64: 1, 128: 1, 1024: 1, 2048: 1, 6016: 0}}
# scene tables staged in LDS (per render, whatever the shape): every small scene; atrium_small is committed as a tree scene of 4-wide nodes and reads them from memory
LDS_STATE = {"cornell_small": 1, "veach_small": 1, "cbox_materials": 1, "atrium_small": 0, "instanced_garden": 1}


def case(mi, oracle, golden_scenes, monkeypatch, name, n=N_PAIRS):
    """per scene, once: the committed scene (under its commit-time switches), the pairs, the oracle's radiance and the anchor shape's result"""
    key = (name, n)
    if key not in _cases:
        clear_knobs(monkeypatch)
        sc = scene_of(mi, golden_scenes, name); env, crit = SCENES.get(name, ({}, "bits"))
        for k, v in env.items(): monkeypatch.setenv(k, v)
        gs = mi.Scene(sc); clear_knobs(monkeypatch)
        pairs = make_pairs(sc, n); ref = oracle.Oracle(sc).render_samples(pairs[:N_PAIRS])["li"]
        r = mi.Render(gs); anchor = r.samples(pairs); info = check_shape(r, n, expect=(-(-n // 64), 64))
        _cases[key] = dict(sc=sc, gs=gs, pairs=pairs, ref=ref, anchor=anchor, crit=crit, info=info)
    clear_knobs(monkeypatch)
    return _cases[key]


def check_vs_oracle(got, ref, crit, tag):
    """the criterion of the scene's own test in tests/test_gpu_parity.py; the figures are printed before they are asserted"""
    share = float((bits(got) == bits(ref)).all(1).mean())
    err = np.abs(got - ref).max(1) / (np.abs(ref).max(1) + 1e-6)
    print(f"[pool-geometry] {tag}: bit share {share:.5f}, err<1e-4 {float((err < 1e-4).mean()):.5f}, median err {float(np.median(err)):.2e}")
    if crit == "bits":
        assert (bits(got) == bits(ref)).all(), (tag, share)
    elif crit == "libm_veach":       # test_roughconductor_veach_mis
        assert (err < 1e-4).mean() > 0.995 and np.median(err) < 1e-6 and share > 0.9999, (tag, share)
    elif crit == "libm_atrium":      # test_envmap_atrium
        assert (err < 1e-4).mean() > 0.99 and np.median(err) < 1e-6 and share > 0.9999, (tag, share)
    else:
        raise AssertionError(crit)
    assert np.isfinite(got).all()


def run_shape(mi, monkeypatch, c, segments, expect=None, grids=None, pairs=None, **render_kw):
    """a fresh render of case c under MI355PT_SEGMENTS (/ MI355PT_GRID_*): its samples and its pool_info, shape asserted"""
    clear_knobs(monkeypatch); grids = grids or {}
    if segments is not None: monkeypatch.setenv("MI355PT_SEGMENTS", str(segments))
    for k, v in grids.items(): monkeypatch.setenv("MI355PT_" + k.upper(), str(v))
    pairs = c["pairs"] if pairs is None else pairs
    r = mi.Render(c["gs"], **render_kw); got = r.samples(pairs); info = check_shape(r, len(pairs), segments, expect, **grids)
    clear_knobs(monkeypatch)
    return got, info


# ---------------------------------------------------------------------------------------------- (a) per-sample radiance under forced shapes
@pytest.mark.parametrize("segments,expect", SEGMENT_ROWS, ids=[f"seg{s}" for s, _ in SEGMENT_ROWS])
@pytest.mark.parametrize("name", list(SCENES))
def test_samples_at_forced_segment_shapes(mi, oracle, golden_scenes, monkeypatch, name, segments, expect):
    """6000 paths in 94 x 64 (anchor), 47 x 128, 6 x 1024, 3 x 2048 and 1 x 6016 slots on the seven scenes that between them run every shade family and ray cast
    (packet + k_shade_d with LDS tables; rough conductors with the class sort; the adapter family; 4-wide tree + fused walk + environment map; instances; both
    volumetric stages): the oracle by the scene's criterion, and the anchor bit for bit, all pairs."""
    c = case(mi, oracle, golden_scenes, monkeypatch, name)
    got, info = run_shape(mi, monkeypatch, c, segments, expect)
    assert info["lds_tables"] == c["info"]["lds_tables"] == LDS_STATE.get(name, info["lds_tables"]), info      # (the volumetric stages have no LDS scene tables to stage)
    if name == "cornell_small": assert info["lds_tables"] == 1 and info["has_roughconductor"] == 0 and info["sorted"] == 0
    if name in ("fog_box", "fog_mis"): assert info["integrator"] in (1, 2) and info["sorted"] == 0
    if name in SORT_STATE: assert info["has_roughconductor"] == 1 and info["sorted"] == SORT_STATE[name][info["cap"]], info
    else: assert info["sorted"] == 0, info
    if name == "veach_small":
        assert info["lds_tables"] == 1 and info["shade_table_bytes"] > 64 * 8 * 64, info      # 64 Sobol dimensions x 8 nibbles x 64 B, then the scene tables
        cls = first_hit_classes(mi, oracle, c)
        occ = occupancy(N_PAIRS, info["n_seg"], info["cap"])
        mixed = [s for s in range(info["n_seg"]) if occ[s] and len(set(cls[s * info["cap"]:s * info["cap"] + occ[s]]) - {-1}) == 2]
        assert mixed, "no segment holds hits of both material classes"
    check_vs_oracle(got, c["ref"], c["crit"], f"{name} {info['n_seg']} x {info['cap']}")
    assert (bits(got) == bits(c["anchor"])).all(), float((bits(got) == bits(c["anchor"])).all(1).mean())


def first_hit_classes(mi, oracle, c):
    """material class of every pair's camera hit: 1 rough conductor (sorted to the back of the order list), 0 anything else, -1 no hit"""
    if "cls" not in c:
        S = mi.scenes; sc = c["sc"]; pos = oracle.Oracle(sc).render_samples(c["pairs"])["pos"]
        rec = c["gs"].ray_intersect(c["gs"].camera_rays(pos))
        rough = np.array([b["type"] == S.BSDF_ROUGHCONDUCTOR for b in sc.bsdfs])
        c["cls"] = np.where(rec["valid"] != 0, rough[np.clip(rec["material"], 0, len(rough) - 1)].astype(np.int64), -1).tolist()
    return c["cls"]


def test_sorted_shading_at_cap_1536(mi, oracle, golden_scenes, monkeypatch):
    """veach_small as the suite renders it (Sobol tables and scene tables in LDS) in 4 x 1536 slots, 24 chunks per segment: the largest row of this file at which its
    order list still fits (3 x 2048 runs unsorted there, SORT_STATE) -- the class sort between cap = 1024 and the independent-sampler case at 4096"""
    c = case(mi, oracle, golden_scenes, monkeypatch, "veach_small")
    got, info = run_shape(mi, monkeypatch, c, 4, (4, 1536))
    assert info["sorted"] == SORT_STATE["veach_small"][1536] == 1 and info["lds_tables"] == 1, info
    check_vs_oracle(got, c["ref"], c["crit"], "veach_small 4 x 1536")
    assert (bits(got) == bits(c["anchor"])).all()


@pytest.mark.parametrize("segments", [None, 6, 1])
def test_samples_with_one_workgroup_per_stage(mi, oracle, golden_scenes, monkeypatch, segments):
    """MI355PT_GRID_EXTEND = _SHADE = _SHADOW = 1: one workgroup strides over all segments of every stage (veach_small: while-while ray cast; sorted shade at 94 x 64 and 6 x 1024, unsorted at 1 x 6016)"""
    c = case(mi, oracle, golden_scenes, monkeypatch, "veach_small")
    got, info = run_shape(mi, monkeypatch, c, segments, grids=dict(grid_extend=1, grid_shade=1, grid_shadow=1))
    assert (info["grid_extend"], info["grid_shade"], info["grid_shadow"]) == (1, 1, 1) and info["sorted"] == SORT_STATE["veach_small"][info["cap"]]
    check_vs_oracle(got, c["ref"], c["crit"], f"veach_small grids 1, {info['n_seg']} x {info['cap']}")
    assert (bits(got) == bits(c["anchor"])).all()


@pytest.mark.parametrize("value", ["0", "-3", "many"])
def test_zero_or_unparsable_overrides_count_as_unset(mi, oracle, golden_scenes, monkeypatch, value):
    """MI355PT_SEGMENTS = 0 used to divide by zero on the host; 0, negative values and non-numbers are now the default rule, for the stage grids as well"""
    c = case(mi, oracle, golden_scenes, monkeypatch, "cornell_small"); clear_knobs(monkeypatch)
    for k in KNOBS[:4]: monkeypatch.setenv(k, value)
    r = mi.Render(c["gs"]); got = r.samples(c["pairs"]); clear_knobs(monkeypatch)
    assert {k: r.pool_info()[k] for k in ("n_seg", "cap", "grid_extend", "grid_shade", "grid_shadow")} == {k: c["info"][k] for k in ("n_seg", "cap", "grid_extend", "grid_shade", "grid_shadow")}
    assert (bits(got) == bits(c["anchor"])).all()


@pytest.mark.parametrize("name", ["cornell_small", "veach_small"])
@pytest.mark.parametrize("paths,segments,expect", BIG_ROWS, ids=["cap10048", "cap70016"])
def test_samples_beyond_the_order_list(mi, oracle, golden_scenes, monkeypatch, name, paths, segments, expect):
    """20000 paths in 2 x 10048 slots (cap > 8192: no order list, rough-conductor scenes shade unsorted) and 70000 in 1 x 70016 (cap > 0xFFFF): the anchor shape of
    the same pairs bit for bit, the oracle on the first 6000 pairs"""
    c = case(mi, oracle, golden_scenes, monkeypatch, name, paths)
    got, info = run_shape(mi, monkeypatch, c, segments, expect)
    assert info["sorted"] == 0 and c["info"]["sorted"] == (1 if name == "veach_small" else 0)
    check_vs_oracle(got[:N_PAIRS], c["ref"], c["crit"], f"{name} {info['n_seg']} x {info['cap']}")
    assert (bits(got) == bits(c["anchor"])).all()


def test_sorted_shading_at_cap_4096(mi, oracle, golden_scenes, monkeypatch):
    """veach_small under the independent sampler (no Sobol tables in LDS): 8100 paths in 2 x 4096 slots, 64 chunks per segment, and the 32 KB order list fits --
    pool_info must say `sorted`.  Reference: the oracle of the same scene description."""
    paths, segments, expect = SORTED_ROW; clear_knobs(monkeypatch)
    S = mi.scenes; sc = S.veach_mis(width=96, height=54, spp=16, sampler=S.SAMPLER_INDEPENDENT, seed=3, max_depth=12)
    pairs = make_pairs(sc, paths); ref = oracle.Oracle(sc).render_samples(pairs[:N_PAIRS])["li"]; gs = mi.Scene(sc)
    r = mi.Render(gs); anchor = r.samples(pairs); check_shape(r, paths, expect=(127, 64))
    c = dict(gs=gs, pairs=pairs)
    got, info = run_shape(mi, monkeypatch, c, segments, expect)
    assert info["sorted"] == 1 and info["has_roughconductor"] == 1
    check_vs_oracle(got[:N_PAIRS], ref, "libm_veach", f"veach independent {info['n_seg']} x {info['cap']}")
    assert (bits(got) == bits(anchor)).all()


# ---------------------------------------------------------------------------------------------- (b) the volumetric 16-bit boundary
@pytest.mark.parametrize("name", ["fog_box", "fog_mis"])
def test_volumetric_segment_of_65472_slots(mi, oracle, golden_scenes, monkeypatch, name):
    """k_shade_vol / k_shade_volmis leave `outS | outE << 16` in shCount[seg]; allocPoolQ keeps a volumetric segment at <= 65472 slots.  Why that is enough (read off
    kernels_vol.hip / kernels_volmis.hip): in one launch a slot i < n sets wantShadow at most once (one emitter-sampling record per vertex) and at most ONE of
    wantSearch / wantAlpha (the `else if`, and one ballot mE = wantSearch | wantAlpha for both), so outS <= n and outE <= n, with n <= cap <= 65472 < 2^16 because
    k_generate fills at most cap slots and the stage only compacts (outA <= n).  65472 = 1023 x 64 is itself a multiple of 64, so rounding cap up to one cannot pass
    it.  Front records go to shBase + [0, outS) with outS <= cap, back records to shBase + 2 cap - 1 - [0, outE) >= shBase + cap: both inside the segment's 2 cap
    record area and disjoint.  So no count overflows and no index leaves the area at cap = 65472 -- nothing to fix; this test pins it: 65472 paths at
    MI355PT_SEGMENTS = 1 run as ONE segment of 1023 chunks, 65473 paths re-grid to 2 x 32768, both bit-equal to the anchor shape for all paths and to the oracle on
    the first 6000."""
    for paths, expect in ((VOL_EDGE, (1, 65472)), (VOL_EDGE + 1, (2, 32768))):
        c = case(mi, oracle, golden_scenes, monkeypatch, name, paths)
        got, info = run_shape(mi, monkeypatch, c, 1, expect)
        check_vs_oracle(got[:N_PAIRS], c["ref"], c["crit"], f"{name} {info['n_seg']} x {info['cap']}")
        assert (bits(got) == bits(c["anchor"])).all()


# ---------------------------------------------------------------------------------------------- (c) films, counters, streams and batches
_films = {}


def film_scene(mi, oracle, name):
    """the 7-spp box-filter scene, its committed handle, the oracle's film and counters"""
    if name not in _films:
        S = mi.scenes; sc = S.cornell_box(96, 54, 7) if name == "cornell_small" else S.fog_box(96, 96, 7)
        ofilm, cnt = oracle.Oracle(sc).render_image(threads=4)
        _films[name] = dict(sc=sc, gs=mi.Scene(sc), ofilm=ofilm, cnt=tuple(int(x) for x in cnt))
    return _films[name]


def one_stream_film(mi, monkeypatch, f):
    if "one" not in f:
        clear_knobs(monkeypatch); monkeypatch.setenv("MI355PT_STREAMS", "1")
        r = mi.Render(f["gs"]); r.run(); assert r.pool_info()["n_pools"] == 1
        f["one"] = r.read_film(0); clear_knobs(monkeypatch)
    return f["one"]


@pytest.mark.parametrize("streams", [1, 2, 3, 4])
@pytest.mark.parametrize("name", ["cornell_small", "fog_box"])
def test_film_over_streams_batches_and_segments(mi, oracle, monkeypatch, name, streams):
    """spp = 7 (nothing divides) over 1..4 pools x planes_per_batch 0 / 1 / 3 x MI355PT_SEGMENTS unset / 5: the film against the oracle's by the box-filter criterion of
    test_film_vs_oracle_and_reference, the three ray counters exactly, and every pixel that received no cross-pixel splat bit-equal to the one-stream film"""
    clear_knobs(monkeypatch); f = film_scene(mi, oracle, name); sc = f["sc"]; one = one_stream_film(mi, monkeypatch, f)
    for ppb in (0, 1, 3):
        for segments in (None, 5):
            clear_knobs(monkeypatch); monkeypatch.setenv("MI355PT_STREAMS", str(streams))
            if segments is not None: monkeypatch.setenv("MI355PT_SEGMENTS", str(segments))
            r = mi.Render(f["gs"], planes_per_batch=ppb); r.run(); film = r.read_film(0); st = r.stats(); info = r.pool_info(); clear_knobs(monkeypatch)
            tag = f"{name} streams {streams} planes {ppb} segments {segments}"
            assert info["n_pools"] == streams, tag
            planes = ppb or -(-7 // streams)      # the batch the pool was sized for: planes_per_batch planes, or the 7 planes cut into one equal batch per pool (mi_render_run_rows)
            want = pool_rule(sc.width * sc.height * planes, info["has_roughconductor"], info["integrator"], segments)
            assert (info["n_seg"], info["cap"]) == (want["n_seg"], want["cap"]), (tag, info, want)
            if segments == 5: assert info["n_seg"] == 5 and info["cap"] > 64
            same = (bits(film) == bits(f["ofilm"])).all(2)
            print(f"[pool-geometry] film {tag}: {float(same.mean()):.5f} of pixels bit-equal to the oracle")
            assert film.shape == f["ofilm"].shape and same.mean() > 0.995 and np.allclose(film, f["ofilm"], rtol=2e-6, atol=1e-7), tag
            assert (st["rays"], st["shadow_rays"], st["path_length_sum"]) == f["cnt"], tag
            # layout 0 = own-pixel sums + spill (cross-pixel splats, float atomics): a pixel whose spill plane is zero is a plain sum in sample order
            clean = (bits(film) == bits(one)).all(2); own = no_spill_pixels(film, one)
            assert clean[own].all() and own.mean() > 0.9, (tag, float(clean.mean()))


def no_spill_pixels(film, one):
    """pixels whose spill plane is zero: every own sample of a pixel adds the same box-filter weight (the discretised filter's value, a little under 1), so such a
    pixel's weight is the sum of spp of them -- the most frequent weight of the film -- or 0 on the border; a splat from a neighbour's sample within 1e-5 of the
    shared edge adds one more"""
    w = film[..., -1]; w1 = one[..., -1]; vals, n = np.unique(w1[w1 > 0], return_counts=True); full = vals[np.argmax(n)]
    return ((w == full) | (w == 0)) & ((w1 == full) | (w1 == 0))


_field_one = {}


@pytest.mark.parametrize("streams", [1, 2, 3, 4])
def test_field_film_over_streams(mi, oracle, monkeypatch, streams):
    """the field film of instanced_garden (37 x 23, 5 spp; one and two planes per batch) over 1..4 pools -- the fieldDone chain exists only with more than one --
    at MI355PT_SEGMENTS unset / 3, compared as test_field_film compares (check_film's rounding bound against the numpy restatement), and -- as for the radiance
    film -- bit for bit with the one-pool field film on every pixel whose spill plane is zero: there the planes are plain sums in sample order, which the fieldDone
    chain has to keep"""
    from tests.test_gpu_fields import film_case, check_film, FILM_FIELDS, UNDEF
    clear_knobs(monkeypatch); sc, gs, exp, mag, cnt, b = film_case(mi, oracle, "instanced_garden", 0)
    if "one" not in _field_one:
        monkeypatch.setenv("MI355PT_STREAMS", "1"); r = mi.Render(gs, planes_per_batch=1, fields=[(f, UNDEF) for f in FILM_FIELDS]); r.run()
        assert r.pool_info()["n_pools"] == 1; _field_one["one"] = r.read_fields(0); clear_knobs(monkeypatch)
    one = _field_one["one"]
    for ppb in (1, 2):
        for segments in (None, 3):
            clear_knobs(monkeypatch); monkeypatch.setenv("MI355PT_STREAMS", str(streams))
            if segments is not None: monkeypatch.setenv("MI355PT_SEGMENTS", str(segments))
            r = mi.Render(gs, planes_per_batch=ppb, fields=[(f, UNDEF) for f in FILM_FIELDS]); r.run(); raw = r.read_fields(0); info = r.pool_info(); clear_knobs(monkeypatch)
            assert info["n_pools"] == streams and (segments is None or (info["n_seg"] == 3 and info["cap"] > 64)), info
            tag = f"instanced_garden streams {streams} planes {ppb} segments {segments}"
            check_film(raw, exp, mag, cnt, tag)
            own = no_spill_pixels(raw, one); clean = (bits(raw) == bits(one)).all(2)      # (the last plane of the field film is the film's weight)
            assert own.mean() > 0.9 and clean[own].all(), (tag, float(own.mean()), float(clean.mean()))


# ---------------------------------------------------------------------------------------------- (d) pool reuse
@pytest.mark.parametrize("name", ["cornell_small", "fog_box"])
def test_pool_reuse_after_growth(mi, oracle, monkeypatch, name):
    """one handle: run() the film (the pool grows to a batch), samples() of 100 pairs in that pool (one part-filled segment, all others empty) = a fresh handle's bit
    for bit; clear() and a quarter tile in the grown pool = a fresh handle's film bit for bit.  MI355PT_SEGMENTS = 40: segments of several chunks."""
    clear_knobs(monkeypatch); f = film_scene(mi, oracle, name); sc = f["sc"]; pairs = make_pairs(sc, 100, seed=7)
    monkeypatch.setenv("MI355PT_SEGMENTS", "40")
    r = mi.Render(f["gs"], planes_per_batch=2); r.run(); grown = r.pool_info(); clear_knobs(monkeypatch)      # (the pool only grows: nothing below allocates on r again)
    assert grown["n_seg"] == 40 and grown["cap"] > 64 and grown["pool_paths"] == sc.width * sc.height * 2
    got = r.samples(pairs); assert r.pool_info() == grown                       # the pool was reused as it is
    fresh = mi.Render(f["gs"]); ref = fresh.samples(pairs); assert fresh.pool_info()["pool_paths"] == 100
    assert (bits(got) == bits(ref)).all() and (bits(got) == bits(oracle.Oracle(sc).render_samples(pairs)["li"])).all()
    tile = (sc.width // 4, sc.height // 4, sc.width // 2 + 1, sc.height // 2 + 1)
    r.clear(); r.run(tile=tile); assert r.pool_info() == grown
    fresh = mi.Render(f["gs"], planes_per_batch=2); fresh.run(tile=tile); assert fresh.pool_info()["pool_paths"] < grown["pool_paths"]
    clear_knobs(monkeypatch)
    a, bfilm = r.read_film(0), fresh.read_film(0)
    assert a.any() and (bits(a) == bits(bfilm)).all()
    assert r.stats()["rays"] == fresh.stats()["rays"]


# ---------------------------------------------------------------------------------------------- (e) one scene, both instantiations
@pytest.mark.parametrize("name", ["cornell_small", "veach_small"])
def test_lds_and_global_tables(mi, oracle, golden_scenes, monkeypatch, name):
    """MI355PT_NO_LDS_TABLES unset / 1 at commit: k_shade<... SMALL ...> against the instantiation that reads the scene tables from memory, at the anchor shape and
    at 6 x 1024 -- bit-equal to each other, to the anchor, and the oracle by the scene's criterion.  Both scenes stage their tables by default (cornell_small: the
    k_shade_d family; veach_small: the rough-conductor family, 140 triangles next to 32 KB of Sobol tables), so pool_info reports 1 against 0 and the launch's LDS in
    front of the order list shrinks to the Sobol tables alone."""
    c = case(mi, oracle, golden_scenes, monkeypatch, name); sc = c["sc"]
    monkeypatch.setenv("MI355PT_NO_LDS_TABLES", "1"); gs = mi.Scene(sc); clear_knobs(monkeypatch)
    for segments in (None, 6):
        got, info = run_shape(mi, monkeypatch, dict(gs=gs, pairs=c["pairs"]), segments)
        assert info["lds_tables"] == 0 and c["info"]["lds_tables"] == 1, (info, c["info"])      # the two settings differ on both scenes
        dims = 4 + 5 * sc.max_depth; assert info["shade_table_bytes"] == dims * 8 * 64 < c["info"]["shade_table_bytes"], (info, c["info"])      # Sobol: dimensions x 8 nibbles x 64 B
        if name == "veach_small": assert info["sorted"] == 1
        check_vs_oracle(got, c["ref"], c["crit"], f"{name} global tables {info['n_seg']} x {info['cap']}")
        assert (bits(got) == bits(c["anchor"])).all()


@pytest.mark.parametrize("name", ["cornell_small", "cbox_lights", "tri_lights", "tri_lights_first_empty"])
def test_table_search_variants(mi, oracle, golden_scenes, monkeypatch, name):
    """MI355PT_SEARCH = 0 .. 3 at commit: cdfSampleReuse's whole-table search (tables of <= 3 bins, its own rules for empty bins) against the binary search + reuse,
    separately for the emitter table (bit 0) and the light-triangle tables (bit 1).  cornell_small: 1 emitter, 2 light triangles; cbox_lights: 3 emitters;
    tri_lights: 3 emitters and a 3-triangle light, each table with a repeated entry (an empty bin at index 1, which no search answers with);
    tri_lights_first_empty: the empty bins come first and pair 0 draws exactly 0, the one input that reaches the rules stepping over an empty bin.  Every setting bit-equal to the others and to the
    oracle: cornell_small and both tri_lights (all diffuse, and the spot -- the one emitter that calls the math library -- has weight 0 and is never drawn) bit for bit,
    cbox_lights by test_scene_level_emitters' criterion."""
    clear_knobs(monkeypatch); sc = scene_of(mi, golden_scenes, name); pairs = make_pairs(sc, N_PAIRS); ref = oracle.Oracle(sc).render_samples(pairs)["li"]
    assert np.isfinite(ref).all() and ref.max() > 0
    results = {}
    for flag in ("0", "1", "2", "3"):
        monkeypatch.setenv("MI355PT_SEARCH", flag); gs = mi.Scene(sc); clear_knobs(monkeypatch)
        for segments in (None, 6):
            got, info = run_shape(mi, monkeypatch, dict(gs=gs, pairs=pairs), segments)
            results[(flag, segments)] = got
            share = float((bits(got) == bits(ref)).all(1).mean()); print(f"[pool-geometry] {name} search {flag} segments {segments}: bit share {share:.5f}")
            if name == "cbox_lights":       # test_scene_level_emitters: the spot light's transition zone calls acosf
                err = np.abs(got - ref).max(1) / (np.abs(ref).max(1) + 1e-6)
                assert share > 0.9999 and (err < 1e-5).mean() > 0.999, (flag, segments, share)
            else:
                assert (bits(got) == bits(ref)).all(), (flag, segments, share)
    first = results[("0", None)]
    for k, v in results.items(): assert (bits(v) == bits(first)).all(), k
