"""CPU: the Python model of the direct integrator (tests/direct_model.py) is pinned to the oracle before anything runs on a GPU.

direct(1,1) IS path with maxDepth = 2 (direct.cpp:146-309 vs path.cpp:119-294): one camera hit, one emitter sample, one BSDF sample, the power heuristic with both
densities scaled by 1/2 (exact in binary floating point).  One difference: direct.cpp requests the emitter side's 2-D sample BEFORE it tests the BSDF for a smooth
component (:210-217), path.cpp after (:172-176).  On a camera hit whose BSDF has no smooth component the BSDF side of `direct` therefore reads Sobol' dimensions
(5, 6) where `path` reads (2, 3).  The bit-for-bit scenes below are chosen so that this cannot show: every BSDF without a smooth component in them is the
zero-reflectance diffuse of the light sources, whose BSDF sample has weight zero whatever the sample.  cbox_materials (smooth conductor, dielectric) is the
scene where it does show."""
import numpy as np
import pytest
from tests.direct_model import DirectModel

W = H = 24; SPP = 4
SPECULAR_SIZE = (48, 48, 8)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def all_pairs():
    return np.array([(x, y, s) for y in range(H) for x in range(W) for s in range(SPP)], np.uint32)


def specular_case(mi):
    """cbox_materials at the smallest size tried (24 x 24 x 4 .. 16, 32 x 32 x 4, 48 x 48 x 8) at which a specular camera hit changes the radiance"""
    w, h, spp = SPECULAR_SIZE; sc = mi.scenes.cbox_materials(w, h, spp, max_depth=2)
    return sc, np.array([(x, y, s) for y in range(h) for x in range(w) for s in range(spp)], np.uint32)


@pytest.fixture(scope="module")
def model_scenes(mi):
    S = mi.scenes
    return {"cornell_box": S.cornell_box(W, H, SPP, max_depth=2), "veach_mis": S.veach_mis(W, H, SPP, max_depth=2), "cbox_materials": S.cbox_materials(W, H, SPP, max_depth=2)}


@pytest.mark.parametrize("name", ["cornell_box", "veach_mis"])
def test_model_11_equals_oracle_path_depth_2(oracle, model_scenes, name):
    sc = model_scenes[name]; pairs = all_pairs()
    ref = oracle.Oracle(sc).render_samples(pairs)["li"]
    got = DirectModel(oracle, sc, 1, 1).render_samples(pairs)
    assert (np.abs(ref).max(1) > 0).mean() > 0.3                  # the scene is lit at this size
    assert (bits(got["li"]) == bits(ref)).all(), float((bits(got["li"]) == bits(ref)).all(1).mean())


def test_model_counts_equal_oracle_path_depth_2(oracle, model_scenes):
    """rays = camera rays + BSDF rays cast, shadow rays = emitter samples with pdf != 0: the counters of the oracle's image loop at maxDepth = 2"""
    sc = model_scenes["cornell_box"]
    _, cnt = oracle.Oracle(sc).render_image()
    got = DirectModel(oracle, sc, 1, 1).render_samples(all_pairs())
    assert (got["rays"], got["shadow_rays"]) == (int(cnt[0]), int(cnt[1]))


def test_model_differs_from_path_only_on_specular_camera_hits(mi, oracle, model_scenes):
    """cbox_materials: smooth conductor, dielectric, plastic.  `path` and direct(1,1) differ exactly where the camera hit has no smooth component: there `direct`
    has consumed the emitter side's sample all the same, so its BSDF side reads dimensions (5, 6) where `path` reads (2, 3).  Checked in both directions on the 2-D
    sample the BSDF side is handed (the oracle logs the values its `path` draws; the last two are the BSDF side's), and in both directions on the radiance: equal
    on every smooth camera hit, different on some specular one.  The radiance shows it rarely: a mirror reflects the same way whatever the sample, and on the glass
    sphere sample.x chooses between reflection and refraction, a refracted ray ends inside the sphere, and only a reflected ray that reaches the light carries
    anything.  At 24 x 24 x 4 no sample does; the radiance is therefore compared at 48 x 48 x 8 (SPECULAR_SIZE), where the geometry guarantees a few."""
    sc = model_scenes["cbox_materials"]; pairs = all_pairs()
    ref = oracle.Oracle(sc).render_samples(pairs, log=True)
    got = DirectModel(oracle, sc, 1, 1).render_samples(pairs)
    spec = got["specular"]; reached = ~np.isnan(got["bsdf_sample"][:, 0])
    assert (spec & reached).sum() > 20 and (~spec & reached).sum() > 20
    nv = ref["nvals"]; assert set(nv[reached & ~spec].tolist()) == {6} and set(nv[reached & spec].tolist()) == {4}     # path: pixel offset, [emitter sample,] BSDF sample
    path_bsdf = np.stack([ref["vals"][np.arange(len(nv)), np.maximum(nv - 2, 0)], ref["vals"][np.arange(len(nv)), np.maximum(nv - 1, 0)]], 1)
    same = (bits(got["bsdf_sample"]) == bits(path_bsdf)).all(1)
    assert same[reached & ~spec].all()                            # equal on every smooth camera hit ...
    assert same[reached & spec].sum() <= 1                        # ... different on every specular one (but the one Sobol' point of index 0, which is 0 in every dimension)
    differs = ~(bits(got["li"]) == bits(ref["li"])).all(1)
    assert not (differs & ~spec).any()                            # a camera hit with a smooth component: the same requests in the same order -> bit for bit
    sc, pairs = specular_case(mi)
    ref = oracle.Oracle(sc).render_samples(pairs)["li"]; got = DirectModel(oracle, sc, 1, 1).render_samples(pairs)
    differs = ~(bits(got["li"]) == bits(ref)).all(1); spec = got["specular"]
    assert not (differs & ~spec).any() and (differs & spec).any()  # ... and the radiance differs on specular camera hits, and only there


@pytest.mark.parametrize("nm", [(4, 0), (0, 4), (3, 2), (4, 4)])
def test_model_converges_to_the_same_image(oracle, model_scenes, nm):
    """an (N, M) estimate has the expectation of the (1, 1) one.  hideEmitters, so that the estimate is the direct lighting alone; the image means agree within 4
    standard errors, each estimated from the estimate's own 2304 samples (the two share camera rays, which only brings them closer).  A wrong weight or a wrong
    fraction in the power heuristic moves the mean by tens of percent."""
    sc = model_scenes["cornell_box"]; pairs = all_pairs()
    a = DirectModel(oracle, sc, 1, 1, hide_emitters=True).render_samples(pairs)["li"].mean(1).astype(np.float64)
    b = DirectModel(oracle, sc, *nm, hide_emitters=True).render_samples(pairs)["li"].mean(1).astype(np.float64)
    se = lambda x: x.std() / np.sqrt(len(x))
    assert a.mean() > 0 and abs(a.mean() - b.mean()) < 4 * np.hypot(se(a), se(b)), (a.mean(), se(a), b.mean(), se(b))
