"""GPU (MI355X): the queue layout of csrc/queues.h -- 12-byte ray / throughput / shadow-contribution records, the ray interval and eta in arrays of their own that
only some launches read, the state of a fresh path a constant of the first shade launch -- at the smallest places where a dropped lane would show.

Every case renders 6000 (pixel, sample) pairs against the oracle by the criterion the scene has in tests/test_gpu_parity.py (bit for bit wherever the scene's own
test is; the criteria are those tests/test_gpu_pool_geometry.py and tests/test_gpu_direct.py quote from there), at the default pool shape (94 x 64 slots) and forced
into 47 x 128, 6 x 1024 and 1 x 6016 slots -- segments of several chunks with a ragged end -- where the forced shapes also equal the default one bit for bit.

  clip planes          Cornell box (packet ray cast, diffuse shade, depth 8), near clip inside the box, far clip in front of the back wall: the camera rays take the
                       interval from the side array, every bounce ray (Epsilon, inf) from the launch
  ... with a thin lens the oracle has no lens: the camera-space depth of every camera hit (the `position` field) lies between the clip planes, the forced shapes equal
                       the default one bit for bit, and the image differs from the one without clip planes
  veach_small          rough conductors: eta through its own array, class-sorted segments
  cbox_materials       smooth dielectric sphere, depth 10 > rrDepth 5: Russian roulette multiplies by an eta != 1 that came through the array
  open_constant        constant environment: st3 next to the re-packed state
  atrium_small         4-wide tree, fused walk, environment map
  instanced_garden     instances
  fog_box / fog_mis    volpath_simple / volpath: rays from medium vertices start at mint = 0, wide shadow records
  direct / ao          on the Cornell box: both write shadow contributions, ao's ray length rides in the shadow origin's fourth lane
  field channels       the field film reads the camera rays by path id"""
import numpy as np
import pytest
from tests.test_gpu_pool_geometry import bits, make_pairs, clear_knobs, check_shape, check_vs_oracle, N_PAIRS
from tests.test_gpu_direct import CRITERIA, rel_err, bit_share

pytestmark = pytest.mark.gpu

SHAPES = [(None, (94, 64)), (47, (47, 128)), (6, (6, 1024)), (1, (1, 6016))]
SHAPE_IDS = ["default", "47x128", "6x1024", "1x6016"]
NEAR, FAR = 900.0, 1300.0      # the Cornell camera sits at z = -800 and looks along +z: the box spans depths 800 .. 1359.2, the short block starts at 865, the back wall is at 1359.2


def clipped_cornell(S, lens=False):
    sc = S.cornell_box(96, 54, 16)
    sc.near, sc.far = NEAR, FAR; sc.sample_to_camera = S.sample_to_camera(sc.xfov, sc.near, sc.far, sc.width / sc.height)
    return S.with_lens(sc, 12.0, 1100.0) if lens else sc


# name -> (scene, commit-time environment, render keywords, criterion, oracle scene or None = the scene itself)
def build_case(mi, golden_scenes, name):
    S = mi.scenes
    if name == "clip": return clipped_cornell(S), {}, {}, "bits", None
    if name == "direct":      # direct(1, 1) is `path` at maxDepth = 2 (tests/test_gpu_direct.py)
        sc = S.cornell_box(96, 54, 16, max_depth=2); return sc, {}, dict(integrator=S.INTEGRATOR_DIRECT, emitter_samples=1, bsdf_samples=1), "bits", None
    env, crit = {"veach_small": ({}, "libm_veach"), "cbox_materials": ({}, "bits"), "open_constant": ({}, "constant"),
                 "atrium_small": ({"MI355PT_BVH2": "0", "MI355PT_NO_PACKET": "1"}, "libm_atrium"), "instanced_garden": ({}, "bits"),
                 "fog_box": ({}, "bits"), "fog_mis": ({}, "bits")}[name]
    return golden_scenes[name], env, {}, crit, None


CASES = ["clip", "veach_small", "cbox_materials", "open_constant", "atrium_small", "instanced_garden", "fog_box", "fog_mis", "direct"]
_cache = {}


def get_case(mi, oracle, golden_scenes, monkeypatch, name):
    """per case, once: the committed scene, the pairs, the oracle's radiance"""
    if name not in _cache:
        clear_knobs(monkeypatch); sc, env, kw, crit, _ = build_case(mi, golden_scenes, name)
        for k, v in env.items(): monkeypatch.setenv(k, v)
        gs = mi.Scene(sc); clear_knobs(monkeypatch)
        pairs = make_pairs(sc, N_PAIRS); ref = oracle.Oracle(sc).render_samples(pairs)["li"]
        _cache[name] = dict(sc=sc, gs=gs, kw=kw, crit=crit, pairs=pairs, ref=ref, results={})
    clear_knobs(monkeypatch)
    return _cache[name]


def render_at(mi, monkeypatch, c, segments, expect):
    """a fresh render of the case under MI355PT_SEGMENTS, its shape asserted; results are kept for the comparison with the default shape"""
    if segments not in c["results"]:
        clear_knobs(monkeypatch)
        if segments is not None: monkeypatch.setenv("MI355PT_SEGMENTS", str(segments))
        r = mi.Render(c["gs"], **c["kw"]); got = r.samples(c["pairs"]); check_shape(r, len(c["pairs"]), segments, expect); clear_knobs(monkeypatch)
        c["results"][segments] = got
    return c["results"][segments]


def judge(got, ref, crit, tag):
    if crit in CRITERIA:
        print(f"[queue-layout] {tag}: bit share {bit_share(got, ref):.5f}, err<1e-4 {float((rel_err(got, ref) < 1e-4).mean()):.5f}, median err {float(np.median(rel_err(got, ref))):.2e}")
        assert CRITERIA[crit](got, ref), tag
        assert np.isfinite(got).all()
    else: check_vs_oracle(got, ref, crit, tag)


@pytest.mark.parametrize("segments,expect", SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("name", CASES)
def test_samples_vs_oracle(mi, oracle, golden_scenes, monkeypatch, name, segments, expect):
    c = get_case(mi, oracle, golden_scenes, monkeypatch, name)
    got = render_at(mi, monkeypatch, c, segments, expect)
    judge(got, c["ref"], c["crit"], f"{name} {expect[0]} x {expect[1]}")
    anchor = render_at(mi, monkeypatch, c, None, SHAPES[0][1])
    assert (bits(got) == bits(anchor)).all(), float((bits(got) == bits(anchor)).all(1).mean())


def test_clip_planes_decide_what_is_seen(mi, oracle, golden_scenes, monkeypatch):
    """the clipped Cornell box is a different picture from the unclipped one (else the case above would not notice a lost interval): camera rays that end in front of the
    back wall see nothing, and the near clip removes the front of the short block; the oracle agrees on which pairs are black.  The back wall (559.2 wide, 1359.2
    from the camera) spans 0.41 of the film's 0.714-wide tangent range and all of its height, the two blocks hide part of it: well over 0.2 of the camera rays end at
    the far plane, on top of the samples that are black in any case (every shadow ray occluded and the path ended)"""
    c = get_case(mi, oracle, golden_scenes, monkeypatch, "clip"); S = mi.scenes
    plain = S.cornell_box(96, 54, 16); got = render_at(mi, monkeypatch, c, None, SHAPES[0][1])
    full = mi.Render(mi.Scene(plain)).samples(c["pairs"])
    black = (got == 0).all(1); black_full = (full == 0).all(1)
    print(f"[queue-layout] clip: {black.mean():.3f} of the pairs black, {black_full.mean():.3f} without the clip planes")
    assert ((c["ref"] == 0).all(1) == black).all() and black_full.mean() + 0.2 < black.mean() < 0.95
    assert (bits(got) != bits(full)).any(1).mean() > 0.2      # (a path whose camera ray ends between the planes is the unclipped path: its bounce rays know no clip plane)


def camera_depth(sc, pos):
    """depth along the camera axis of world positions [n, 3] (cam_to_world is a rigid transform here)"""
    m = np.asarray(sc.cam_to_world, np.float64); return (pos.astype(np.float64) - m[:3, 3]) @ m[:3, 2]


@pytest.mark.parametrize("segments,expect", SHAPES, ids=SHAPE_IDS)
def test_clip_planes_with_a_thin_lens(mi, monkeypatch, segments, expect):
    """lensRay derives (mint, maxt) from the clip planes per aperture sample.  The oracle has no lens, so: every camera hit lies between the planes (depth of the
    `position` field along the camera axis, within the rounding of t = depth / cos), some camera rays find nothing, the image is not the unclipped one, and the
    forced shapes equal the default one bit for bit"""
    key = "clip_lens"
    if key not in _cache:
        clear_knobs(monkeypatch); S = mi.scenes; sc = clipped_cornell(S, lens=True); gs = mi.Scene(sc); pairs = make_pairs(sc, N_PAIRS)
        r = mi.Render(gs, fields=[("position", (0.0, 0.0, -1e9))]); pos = r.field_samples(pairs)[:, 0, :]
        plain = S.with_lens(S.cornell_box(96, 54, 16), 12.0, 1100.0); full = mi.Render(mi.Scene(plain)).samples(pairs)
        _cache[key] = dict(sc=sc, gs=gs, kw={}, pairs=pairs, pos=pos, full=full, results={})
    c = _cache[key]; clear_knobs(monkeypatch)
    got = render_at(mi, monkeypatch, c, segments, expect); anchor = render_at(mi, monkeypatch, c, None, SHAPES[0][1])
    assert (bits(got) == bits(anchor)).all() and np.isfinite(got).all()
    hit = c["pos"][:, 2] > -1e8; depth = camera_depth(c["sc"], c["pos"][hit])
    print(f"[queue-layout] clip + lens {expect}: {hit.mean():.3f} of the camera rays hit, depth {depth.min():.2f} .. {depth.max():.2f}")
    assert 0.05 < hit.mean() < 0.95 and depth.min() >= NEAR * (1 - 1e-5) and depth.max() <= FAR * (1 + 1e-5)
    assert (got[~hit] == 0).all() and (got[hit] > 0).any(1).mean() > 0.5      # a camera ray that finds nothing between the planes adds nothing (no environment)
    assert (bits(got) != bits(c["full"])).any(1).mean() > 0.2      # the share of the film the back wall fills (test_clip_planes_decide_what_is_seen)


@pytest.mark.parametrize("segments,expect", SHAPES, ids=SHAPE_IDS)
def test_ao_vs_model(mi, oracle, monkeypatch, segments, expect):
    """ao(4) on the Cornell box against the Python model of ao.cpp (tests/ao_model.py), bit for bit: contribution (1,1,1) in the 12-byte record, the ray length in shO.w"""
    from tests.ao_model import AoModel
    key = "ao"
    if key not in _cache:
        clear_knobs(monkeypatch); S = mi.scenes; sc = S.cornell_box(48, 32, 4, max_depth=2); pairs = make_pairs(sc, N_PAIRS)
        model = AoModel(oracle, sc, 4, 300.0).render_samples(pairs)
        _cache[key] = dict(sc=sc, gs=mi.Scene(sc), kw=dict(integrator=S.INTEGRATOR_AO, shading_samples=4, ray_length=300.0), pairs=pairs, ref=model["li"], hit=model["hit"], results={})
    c = _cache[key]; clear_knobs(monkeypatch)
    got = render_at(mi, monkeypatch, c, segments, expect)
    assert c["hit"].mean() > 0.2 and 0.05 < c["ref"][c["hit"]].mean() < 0.999      # the scene is in the picture, and so is the occlusion at this ray length
    assert (bits(got) == bits(c["ref"])).all(), bit_share(got, c["ref"])


@pytest.mark.parametrize("segments", [None, 3])
def test_field_film(mi, oracle, monkeypatch, segments):
    """the field film of instanced_garden (tests/test_gpu_fields.py: 37 x 23, 5 spp against the numpy restatement of ImageBlock::put): kernels_field.hip rebuilds the
    camera hit from the ray origin and direction of path `pid`"""
    from tests.test_gpu_fields import film_case, check_film, FILM_FIELDS, UNDEF
    clear_knobs(monkeypatch); sc, gs, exp, mag, cnt, b = film_case(mi, oracle, "instanced_garden", 0)
    if segments is not None: monkeypatch.setenv("MI355PT_SEGMENTS", str(segments))
    r = mi.Render(gs, planes_per_batch=2, fields=[(f, UNDEF) for f in FILM_FIELDS]); r.run(); raw = r.read_fields(0); info = r.pool_info(); clear_knobs(monkeypatch)
    assert segments is None or (info["n_seg"] == 3 and info["cap"] > 64), info
    check_film(raw, exp, mag, cnt, f"instanced_garden segments {segments}")
