"""GPU (MI355X): the HIP path, called through the C-ABI (include/mi355pt.h via mitsuba-im_amd/api.py), against the oracle
on the same seeded inputs, against the golden fixtures of the reference, and -- at BASELINE sizes -- through size-independent
properties (tile/sample-range additivity, determinism, weight channel, ray counters)."""
import os
import numpy as np
import pytest
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu


def bit_share(got, ref, tag):
    """share of samples whose three channels equal the oracle's bit for bit; printed (pytest -s) so that the floors asserted in the tests can be checked against measured values"""
    share = float((bits(got) == bits(ref)).all(1).mean())
    print(f"[bit-share] {tag}: {share:.4f}")      # round 3 on MI355X, device library's libm: analytic_shapes 0.9897 / 0.9956, instances 0.9957, thin_dielectric 0.9887 / 0.9922, mask 0.9942 / 0.9932,
    return share                                   # tree_node_kinds atrium_small 0.8276; with glibc's routines restated on the device (csrc/libm_glibc.h): 1.0000 in every one -- the floors are 0.9999


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def scenes(mi):
    S = mi.scenes
    return {
        "cornell_sobol": S.cornell_box(1920, 1080, 8),
        "cornell_indep": S.cornell_box(1920, 1080, 8, sampler=S.SAMPLER_INDEPENDENT, seed=0),
        "cornell_indep_seed5": S.cornell_box(640, 360, 4, sampler=S.SAMPLER_INDEPENDENT, seed=5),
        "cornell_depth12": S.cornell_box(512, 288, 4, max_depth=12, rr_depth=3),
        "closed_box": S.closed_box(),
    }


@pytest.mark.parametrize("name", ["cornell_sobol", "cornell_indep", "cornell_indep_seed5", "cornell_depth12", "closed_box"])
def test_li_samples_bit_exact_vs_oracle(mi, oracle, scenes, name):
    """Bit-exact: integer sampler math AND the fp32 radiance (DESIGN.md arithmetic contract)."""
    sc = scenes[name]; rng = np.random.default_rng(11); n = 30000
    pairs = np.stack([rng.integers(0, sc.width, n), rng.integers(0, sc.height, n), rng.integers(0, sc.spp, n)], 1).astype(np.uint32)
    pairs[:4] = [[0, 0, 0], [sc.width - 1, sc.height - 1, sc.spp - 1], [sc.width - 1, 0, 0], [0, sc.height - 1, sc.spp - 1]]
    ref = oracle.Oracle(sc).render_samples(pairs)["li"]
    r = mi.Render(mi.Scene(sc)); got = r.samples(pairs)
    assert (bits(got) == bits(ref)).all()


@pytest.mark.parametrize("name", ["cornell_sobol", "cornell_indep", "cornell_small", "cornell_small_gauss"])
def test_li_samples_vs_reference_golden(mi, golden_scenes, name):
    """Against the REFERENCE's own Li (fixtures from the compiled reference): tolerance 2e-4 relative per sample (-ffast-math reference)."""
    sc = golden_scenes[name]; gd = np.load(os.path.join(GOLDEN, name + "_samples.npz"))
    got = mi.Render(mi.Scene(sc)).samples(gd["pairs"])
    err = np.abs(got - gd["li"]).max(1) / (np.abs(gd["li"]).max(1) + 1e-6)
    assert (err < 2e-4).mean() > 0.995 and err.max() < 5e-3 and np.median(err) < 1e-6
    # ... and against the SAME reference sources compiled without -ffast-math (tests/golden/strict/): bit for bit
    st = np.load(os.path.join(GOLDEN, "strict", name + ".npz"))
    assert (bits(got) == bits(st["li"])).all()


def test_sobol_and_camera_units(mi, oracle, scenes):
    sc = scenes["cornell_sobol"]; gs = mi.Scene(sc); orc = oracle.Oracle(sc); L = oracle.lib()
    rng = np.random.default_rng(3); n = 4096
    q = np.stack([rng.integers(0, sc.width, n), rng.integers(0, sc.height, n), rng.integers(0, 256, n)], 1).astype(np.uint32)
    idx, vals = gs.sobol(q, 40)
    for i in range(0, n, 37):
        ref_idx = L.orc_sobol_look_up(orc.h, 11, int(q[i, 2]), int(q[i, 0]), int(q[i, 1]))
        assert idx[i] == ref_idx
        for d in (0, 1, 4, 5, 17, 39):
            assert vals[i, d] == np.float32(L.orc_sobol_sample(orc.h, ref_idx, d))
    # 4K film (BASELINE configs 4/5): resolution 4096 -> m = 12, 1024 spp -> 34-bit indices (9 nibble lookups)
    sc4 = mi.scenes.cornell_box(3840, 2160, 1024); gs4 = mi.Scene(sc4); orc4 = oracle.Oracle(sc4)
    q4 = np.stack([rng.integers(0, 3840, 2048), rng.integers(0, 2160, 2048), rng.integers(0, 1024, 2048)], 1).astype(np.uint32)
    idx4, vals4 = gs4.sobol(q4, 44)
    for i in range(0, 2048, 19):
        ref_idx = L.orc_sobol_look_up(orc4.h, 12, int(q4[i, 2]), int(q4[i, 0]), int(q4[i, 1]))
        assert idx4[i] == ref_idx and ref_idx < (1 << 34)
        for d in (0, 1, 5, 43):
            assert vals4[i, d] == np.float32(L.orc_sobol_sample(orc4.h, ref_idx, d))
    li4 = mi.Render(gs4).samples(q4[:512]); ref4 = orc4.render_samples(q4[:512])["li"]
    assert (bits(li4) == bits(ref4)).all()
    # golden Sobol vectors of the reference (m = 2, 7, 12 tables are exercised on the oracle side; here m = 11 via look_up above)
    pos = rng.random((512, 2)).astype(np.float32) * np.array([sc.width, sc.height], np.float32)
    rays = gs.camera_rays(pos)
    for i in range(512):
        assert (bits(rays[i]) == bits(orc.camera_ray(float(pos[i, 0]), float(pos[i, 1])))).all()


@pytest.mark.parametrize("name", ["cornell_sobol", "closed_box"])
def test_intersection_bit_exact(mi, oracle, scenes, name):
    sc = scenes[name]; gs = mi.Scene(sc); orc = oracle.Oracle(sc); rng = np.random.default_rng(5); n = 3000
    lo, hi = sc.pos.min(0) - 5, sc.pos.max(0) + 5
    o = (lo + rng.random((n, 3)) * (hi - lo)).astype(np.float32)
    d = rng.normal(size=(n, 3)); d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    d[:50, 0] = 0; d[50:100, 1] = 0; d[100:110] = [0, 0, 1]       # axis-parallel rays (zero components)
    rays = np.concatenate([o, np.full((n, 1), 1e-4, np.float32), d, np.full((n, 1), np.inf, np.float32)], 1).astype(np.float32)
    rays[200:400, 7] = rng.random(200) * 300                       # finite maxt
    got = gs.intersect(rays); occ = gs.intersect(rays, any_hit=True)
    nhit = 0
    for i in range(n):
        ok, h = orc.intersect(rays[i])
        assert ok == (got[i, 3] >= 0)
        if ok:
            nhit += 1
            # t, u, v bit-exact; prim = global triangle index
            assert (bits(got[i, :3]) == bits(np.array([h[0], h[13], h[14]], np.float32))).all()
            shape = int(h[19]); assert int(got[i, 3]) == sc.shapes[shape]["first_tri"] + int(h[18])
        assert orc.occluded(rays[i]) == (occ[i, 3] >= 0)
    assert nhit > n // 20


@pytest.mark.parametrize("name", ["cornell_sobol", "closed_box", "veach_small"])
def test_packet_candidate_search_is_conservative(mi, oracle, golden_scenes, scenes, name):
    """Packet mode (trace.h): pass 1 marks candidate triangles with an approximate, margin-padded test, pass 2 runs the exact Wald test on them.  A false
    negative of pass 1 would change (t, u, v, prim), so aim rays where the margins matter: exactly at vertices and at points on edges (from random origins
    and from origins ON other surfaces), grazing along the planes of the triangles (|D| small), through the quad diagonals, with mint / maxt ending right at
    the hit.  Compared bit for bit with the oracle's test over ALL triangles (veach_small: the same rays through the BVH path)."""
    sc = (golden_scenes if name == "veach_small" else scenes)[name]; gs = mi.Scene(sc); orc = oracle.Oracle(sc); rng = np.random.default_rng(17)
    P = sc.pos[sc.idx.reshape(-1, 3)].astype(np.float64)                      # (nt, 3, 3)
    nt = len(P); lo, hi = sc.pos.min(0), sc.pos.max(0); ext = (hi - lo).max()
    rays = []
    for rep in range(24 * max(1, 192 // nt)):
        t = rng.integers(0, nt, nt); w = rng.dirichlet([1, 1, 1], nt)
        for kind in range(6):
            if kind == 0: target = P[t, rng.integers(0, 3, nt)]                                    # a vertex
            elif kind == 1: a = rng.random((nt, 1)); e = rng.integers(0, 3, nt); target = P[t, e] * a + P[t, (e + 1) % 3] * (1 - a)      # a point on an edge
            elif kind == 2: target = (P[t] * w[:, :, None]).sum(1)                                 # an interior point
            elif kind == 3: target = (P[t, 0] + P[t, 1] + P[t, 2]) / 3 + (P[t, 1] - P[t, 0]) * 1e-4      # next to the centroid
            elif kind == 4: a = rng.random((nt, 1)); target = P[t, 1] * a + P[t, 2] * (1 - a) + (P[t, 0] - P[t, 1]) * 1e-6 * rng.normal(size=(nt, 1))   # within 1e-6 of the edge opposite vertex 0
            else: target = P[t, 0] + (P[t, 1] - P[t, 0]) * rng.random((nt, 1)) * 3 - (P[t, 2] - P[t, 0]) * rng.random((nt, 1))      # in the plane, mostly outside
            if rep % 3 == 0: o = lo + rng.random((nt, 3)) * (hi - lo)                              # origin inside the scene box
            elif rep % 3 == 1:
                t2 = rng.integers(0, nt, nt); o = (P[t2] * rng.dirichlet([1, 1, 1], nt)[:, :, None]).sum(1)      # origin ON another surface
            else:                                                                                   # grazing: origin (almost) in the target triangle's plane
                nrm = np.cross(P[t, 1] - P[t, 0], P[t, 2] - P[t, 0]); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True) + 1e-30
                side = P[t, 0] + (P[t, 1] - P[t, 0]) * (rng.random((nt, 1)) * 4 - 2) + (P[t, 2] - P[t, 0]) * (rng.random((nt, 1)) * 4 - 2)
                o = side + nrm * ext * 10.0 ** rng.uniform(-7, -2, (nt, 1)) * rng.choice([-1, 1], (nt, 1))
            d = target - o; ln = np.linalg.norm(d, axis=1, keepdims=True); ok = ln[:, 0] > 1e-9
            d = d / np.maximum(ln, 1e-30)
            mint = np.full(nt, 1e-4); maxt = np.full(nt, np.inf)
            if rep % 4 == 3: maxt = ln[:, 0] * (1 + rng.choice([-1e-6, 0, 1e-6], nt))             # the interval ends (almost) at the target
            rays.append(np.concatenate([o, mint[:, None], d, maxt[:, None]], 1)[ok])
    rays = np.concatenate(rays).astype(np.float32)
    got = gs.intersect(rays); occ = gs.intersect(rays, any_hit=True)
    nhit = 0
    for i in range(len(rays)):
        ok, h = orc.intersect(rays[i])
        assert ok == (got[i, 3] >= 0), (i, rays[i])
        if ok:
            nhit += 1
            assert (bits(got[i, :3]) == bits(np.array([h[0], h[13], h[14]], np.float32))).all(), (i, rays[i])
            assert int(got[i, 3]) == sc.shapes[int(h[19])]["first_tri"] + int(h[18]), (i, rays[i])
        assert orc.occluded(rays[i]) == (occ[i, 3] >= 0), (i, rays[i])
    assert nhit > len(rays) // 4


@pytest.mark.parametrize("name,spp", [("cornell_small", 16), ("cornell_small_gauss", 4), ("closed_box", 16), ("cornell_small_tent", 4),
                                      ("cornell_small_mitchell", 4), ("cornell_small_catmullrom", 4), ("cornell_small_lanczos", 4)])
def test_film_vs_oracle_and_reference(mi, oracle, golden_scenes, name, spp):
    sc = golden_scenes[name]
    r = mi.Render(mi.Scene(sc)); r.run(); film = r.read_film(0); st = r.stats()
    ofilm, cnt = oracle.Oracle(sc).render_image(threads=4)
    assert film.shape == ofilm.shape
    if sc.filter == 0:
        # box filter: every pixel sums its own samples in sample order -> bit-exact, except pixels that received a spill from a
        # neighbour's sample sitting within 1e-5 of the shared edge (added separately, float atomics): allow those 1e-6 relative
        same = (bits(film) == bits(ofilm)).all(2)
        assert same.mean() > 0.995 and np.allclose(film, ofilm, rtol=2e-6, atol=1e-7)
    else:
        assert np.allclose(film, ofilm, rtol=2e-5, atol=2e-6)       # wider filters: all splats are float atomics (negative lobes cancel: absolute tolerance)
    assert (st["rays"], st["shadow_rays"], st["path_length_sum"]) == tuple(int(c) for c in cnt)
    ref = np.load(os.path.join(GOLDEN, name + "_image.npz"))["film"]
    rel = np.linalg.norm(film[..., :3] - ref[..., :3]) / np.linalg.norm(ref[..., :3])
    assert rel < (2e-2 if name == "closed_box" else 1e-4), rel
    # developed image = sum / weight (hdrfilm.cpp:352,396) and the responsive RGBA layout
    dev = r.read_film(2); b = r.film_shape(0)[3]
    inner = film[b:film.shape[0] - b, b:film.shape[1] - b]
    assert np.allclose(dev, inner[..., :3] / inner[..., 4:5], rtol=1e-6)
    assert (bits(r.read_film(1)) == bits(film[..., :4])).all()


def test_full_size_properties(mi, scenes):
    """BASELINE size (1920x1080, Sobol, depth 8): properties that need no CPU oracle."""
    sc = scenes["cornell_sobol"]; gs = mi.Scene(sc); r = mi.Render(gs, spp=8)
    r.run(); full = r.read_film(0); st = r.stats()
    n = 1920 * 1080 * 8
    assert st["samples"] == n and 3.5 < st["rays"] / n < 6.5 and 1.5 < st["shadow_rays"] / n < 4.0
    assert np.isfinite(full).all() and (full >= 0).all()
    # weight channel: every pixel received exactly spp samples of weight ~1 (box table value), border ~0
    # (a sample within 1e-5 of a pixel edge splats into both pixels -- box radius 0.5+1e-5, src/rfilters/box.cpp:38; Sobol' points of low
    # index sit exactly on dyadic pixel fractions, so ~0.2 % of the pixels hold one more)
    w = full[1:-1, 1:-1, 4]; w0 = np.median(w)
    assert abs(w0 / 8 - 1) < 1e-3 and np.isclose(w, w0, rtol=1e-4).mean() > 0.99
    extra = np.round((w - w0) / (w0 / 8)); assert (extra >= 0).all() and extra.max() <= 3 and np.allclose(w, w0 + extra * (w0 / 8), rtol=1e-4)
    # determinism
    r.clear(); r.run(); again = r.read_film(0)
    assert (bits(again[1:-1, 1:-1]) == bits(full[1:-1, 1:-1])).mean() > 0.995
    # additivity over sample ranges and over tiles (global pixel coordinates in the sampler: SURVEY.md §7 look_up)
    r.clear(); r.run(s0=0, s1=3); r.run(s0=3, s1=8); parts = r.read_film(0)
    assert np.allclose(parts, full, rtol=1e-5, atol=1e-6)
    r.clear()
    for tile in [(0, 0, 1920, 500), (0, 500, 700, 1080), (700, 500, 1920, 1080)]:
        r.run(tile=tile)
    tiles = r.read_film(0)
    assert (bits(tiles[1:-1, 1:-1]) == bits(full[1:-1, 1:-1])).mean() > 0.995 and np.allclose(tiles, full, rtol=1e-5, atol=1e-6)
    # rows interleaved over 3 "ranks" (mi_render_run_rows): the union is the full frame
    r.clear()
    for k in range(3):
        r.run(tile=(0, k, 1920, 1080), row_stride=3)
    inter = r.read_film(0)
    assert (bits(inter[1:-1, 1:-1]) == bits(full[1:-1, 1:-1])).mean() > 0.995 and np.allclose(inter, full, rtol=1e-5, atol=1e-6)
    # batching must not change the result
    r2 = mi.Render(gs, spp=8, planes_per_batch=1); r2.run(); one = r2.read_film(0)
    assert (bits(one[1:-1, 1:-1]) == bits(full[1:-1, 1:-1])).mean() > 0.995


def test_edge_cases_and_errors(mi, scenes):
    S = mi.scenes
    # ragged tiny films, 1 sample, maxDepth 1
    for w, h, spp, md in [(1, 1, 1, 8), (3, 2, 1, 1), (257, 3, 2, 2)]:
        sc = S.cornell_box(w, h, spp, max_depth=md); r = mi.Render(mi.Scene(sc)); r.run(); f = r.read_film(0)
        assert np.isfinite(f).all() and abs(f[1:-1, 1:-1, 4].mean() / spp - 1) < 1e-3
        if md == 1:
            assert r.stats()["shadow_rays"] == 0
    sc = scenes["cornell_depth12"]; gs = mi.Scene(sc)
    with pytest.raises(mi.MiError, match="rrDepth"):
        mi.Render(gs, rr_depth=0)
    with pytest.raises(mi.MiError, match="maxDepth"):
        mi.Render(gs, max_depth=0)
    r = mi.Render(gs)
    with pytest.raises(mi.MiError, match="tile"):
        r.run(tile=(0, 0, sc.width + 1, 10))
    with pytest.raises(mi.MiError, match="sample range"):
        r.run(s0=0, s1=sc.spp + 1)
    # Integrator::cancel: a cancel issued between two runs is not lost -- the next run sees it, returns MI_CANCELLED and consumes it
    r.clear(); r.cancel()
    with pytest.raises(mi.MiError, match="cancelled"):
        r.run()
    assert r.stats()["samples"] == 0
    r.run(); assert r.stats()["samples"] > 0
    r.cancel(); r.clear(); r.run(); assert r.stats()["samples"] > 0        # mi_render_clear drops a pending cancel


def test_independent_stream_period_is_refused(mi, golden_scenes):
    """the build-defined independent stream numbers a path's draws with 8 bits: a maxDepth that could draw more than 256 values is refused by name"""
    S = mi.scenes; gs = mi.Scene(golden_scenes["cornell_small"])
    mi.Render(gs, sampler=S.SAMPLER_INDEPENDENT, max_depth=50).run(s1=1)      # 2 + 5 * 50 = 252
    with pytest.raises(RuntimeError, match="independent sampler stream"):
        mi.Render(gs, sampler=S.SAMPLER_INDEPENDENT, max_depth=51)


def test_opacity_alpha_channel(mi, oracle, golden_scenes):
    """EOpacity (records.inl:121-137): alpha = 1 where the camera ray hits, 0 where it leaves the scene; off -> alpha = 1 everywhere."""
    sc = golden_scenes["cornell_small"]
    r = mi.Render(mi.Scene(sc), opacity=True); r.run(); film = r.read_film(0)
    ofilm, _ = oracle.Oracle(sc, opacity=True).render_image(threads=4)
    assert np.allclose(film, ofilm, rtol=2e-6, atol=1e-7) and (bits(film) == bits(ofilm)).all(2).mean() > 0.99
    assert film[1:-1, 1:-1, 3].min() < 0.5 * film[1:-1, 1:-1, 4].max()      # some camera rays miss at the left/right film edge
    r2 = mi.Render(mi.Scene(sc)); r2.run(); f2 = r2.read_film(0)
    assert np.allclose(f2[..., 3], f2[..., 4]) and np.allclose(f2[..., :3], film[..., :3], rtol=2e-6, atol=1e-7)


def test_roughconductor_veach_mis(mi, oracle, golden_scenes):
    """S2 (BASELINE config 3 at test size): twosided(roughconductor) plates + disc lights, maxDepth 12, BVH traversal (142 triangles).
    The microfacet code calls exp/log/acos/atan2/tan/sin/cos/pow from the device math library vs libm in the oracle, so this BSDF is
    tolerance-pinned: 1e-4 relative per sample for >= 99.5 % of the samples (the rest are paths that fork on a last-bit difference)."""
    sc = golden_scenes["veach_small"]; gs = mi.Scene(sc); r = mi.Render(gs)
    rng = np.random.default_rng(21); n = 20000
    pairs = np.stack([rng.integers(0, sc.width, n), rng.integers(0, sc.height, n), rng.integers(0, sc.spp, n)], 1).astype(np.uint32)
    ref = oracle.Oracle(sc).render_samples(pairs)["li"]; got = r.samples(pairs)
    err = np.abs(got - ref).max(1) / (np.abs(ref).max(1) + 1e-6)
    assert (err < 1e-4).mean() > 0.995 and np.median(err) < 1e-6, ((err < 1e-4).mean(), np.median(err))
    assert bit_share(got, ref, "veach_small") > 0.9999      # glibc's libm restated on the device: the microfacet scene equals the oracle bit for bit
    gd = np.load(os.path.join(GOLDEN, "veach_small_samples.npz"))            # the reference's own Li
    got = r.samples(gd["pairs"]); err = np.abs(got - gd["li"]).max(1) / (np.abs(gd["li"]).max(1) + 1e-6)
    assert (err < 2e-4).mean() > 0.995 and np.median(err) < 1e-6
    r.run(); film = r.read_film(0); st = r.stats()
    ofilm, cnt = oracle.Oracle(sc).render_image(threads=4)
    rel = np.linalg.norm(film[..., :3] - ofilm[..., :3]) / np.linalg.norm(ofilm[..., :3])
    print(f"[film-rel] veach_small: {rel:.3e} rays {st['rays']} vs {int(cnt[0])} shadow {st['shadow_rays']} vs {int(cnt[1])}")
    assert rel < 1e-6, rel                                                   # (round 2: 2e-3 -- a forked path moved a whole pixel; round 3: no path forks any more)
    assert st["rays"] == int(cnt[0]) and st["shadow_rays"] == int(cnt[1])
    ref_film = np.load(os.path.join(GOLDEN, "veach_small_image.npz"))["film"]
    assert np.linalg.norm(film[..., :3] - ref_film[..., :3]) / np.linalg.norm(ref_film[..., :3]) < 2e-3


def test_envmap_atrium(mi, oracle, golden_scenes):
    """S3 at test size (BASELINE configs 4/5): environment emitter + area lanterns (emitter selection CDF), smooth-shaded columns,
    twosided walls.  atan2/acos/sin/cos of the lat-long lookups come from the device math library -> tolerance-pinned."""
    sc = golden_scenes["atrium_small"]; gs = mi.Scene(sc); r = mi.Render(gs)
    rng = np.random.default_rng(31); n = 20000
    pairs = np.stack([rng.integers(0, sc.width, n), rng.integers(0, sc.height, n), rng.integers(0, sc.spp, n)], 1).astype(np.uint32)
    ref = oracle.Oracle(sc).render_samples(pairs)["li"]; got = r.samples(pairs)
    err = np.abs(got - ref).max(1) / (np.abs(ref).max(1) + 1e-6)
    assert (err < 1e-4).mean() > 0.99 and np.median(err) < 1e-6, ((err < 1e-4).mean(), np.median(err))
    assert bit_share(got, ref, "atrium_small") > 0.9999      # atan2f / acosf of the lat-long lookups = glibc's: bit-exact
    gd = np.load(os.path.join(GOLDEN, "atrium_small_samples.npz"))           # the reference's own Li
    got = r.samples(gd["pairs"]); err = np.abs(got - gd["li"]).max(1) / (np.abs(gd["li"]).max(1) + 1e-6)
    assert (err < 1e-4).mean() > 0.97 and (err < 1e-2).mean() > 0.995 and np.median(err) < 1e-6
    r.run(); film = r.read_film(0); ofilm, cnt = oracle.Oracle(sc).render_image(threads=4); st = r.stats()
    print(f"[film-rel] atrium_small: {np.linalg.norm(film[..., :3] - ofilm[..., :3]) / np.linalg.norm(ofilm[..., :3]):.3e} rays {st['rays']} vs {int(cnt[0])}")
    assert np.linalg.norm(film[..., :3] - ofilm[..., :3]) / np.linalg.norm(ofilm[..., :3]) < 1e-6
    assert st["rays"] == int(cnt[0])
    assert film[1:-1, 1:-1, :3].mean() > 0.05                               # the sky actually lights the scene


def test_large_scene_bvh_vs_oracle(mi, oracle):
    """~40 k triangles (deeper BVH, LDS stack variants): closest-hit (t, u, v, prim) bit-exact and any-hit equal to the oracle's own BVH."""
    sc = mi.scenes.atrium(64, 36, 1, detail=0.4, env_size=(64, 32)); gs = mi.Scene(sc); orc = oracle.Oracle(sc)
    assert len(sc.idx) > 30000
    rng = np.random.default_rng(9); n = 4000
    lo, hi = sc.pos.min(0), sc.pos.max(0)
    o = (lo + rng.random((n, 3)) * (hi - lo)).astype(np.float32); o[:, 1] = np.abs(o[:, 1]) * 0.9 + 0.05
    d = rng.normal(size=(n, 3)); d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    rays = np.concatenate([o, np.full((n, 1), 1e-4, np.float32), d, np.full((n, 1), np.inf, np.float32)], 1).astype(np.float32)
    got = gs.intersect(rays); occ = gs.intersect(rays, any_hit=True)
    for i in range(n):
        ok, h = orc.intersect(rays[i])
        assert ok == (got[i, 3] >= 0)
        if ok:
            assert (bits(got[i, :3]) == bits(np.array([h[0], h[13], h[14]], np.float32))).all()
            assert int(got[i, 3]) == sc.shapes[int(h[19])]["first_tri"] + int(h[18])
        assert orc.occluded(rays[i]) == (occ[i, 3] >= 0)


@pytest.mark.parametrize("name", ["atrium_strict", "atrium_hide_indep", "cornell_hide"])
def test_integrator_switches(mi, oracle, golden_scenes, name):
    """strictNormals, hideEmitters, early Russian roulette (rrDepth 1..3), unbounded depth (maxDepth = -1, independent stream)."""
    sc = golden_scenes[name]; r = mi.Render(mi.Scene(sc))
    gd = np.load(os.path.join(GOLDEN, name + "_samples.npz")); pairs = gd["pairs"]
    o = oracle.Oracle(sc).render_samples(pairs); got = r.samples(pairs)
    if name == "cornell_hide":
        assert (bits(got) == bits(o["li"])).all()
        err = np.abs(got - gd["li"]).max(1) / (np.abs(gd["li"]).max(1) + 1e-6); assert err.max() < 2e-4
    else:
        err = np.abs(got - o["li"]).max(1) / (np.abs(o["li"]).max(1) + 1e-6)
        assert (err < 1e-4).mean() > 0.99 and np.median(err) < 1e-6
        assert bit_share(got, o["li"], "integrator_switches " + name) > 0.9999
        err = np.abs(got - gd["li"]).max(1) / (np.abs(gd["li"]).max(1) + 1e-6)
        assert (err < 1e-4).mean() > 0.97 and (err < 1e-2).mean() > 0.995
    r.run(); film = r.read_film(0); ofilm, cnt = oracle.Oracle(sc).render_image(threads=4); st = r.stats()
    assert np.linalg.norm(film[..., :3] - ofilm[..., :3]) / np.linalg.norm(ofilm[..., :3]) < 3e-3
    assert abs(st["rays"] - int(cnt[0])) / cnt[0] < 2e-3 and abs(st["path_length_sum"] - int(cnt[2])) / cnt[2] < 2e-3


@pytest.mark.parametrize("name", ["cbox_shapes", "shape_lights", "cbox_shapes_strict_indep"])
@pytest.mark.parametrize("bvh", [False, True])
def test_analytic_shapes(mi, oracle, golden_scenes, name, bvh, monkeypatch):
    """rectangle / disk / sphere / cylinder behind rayIntersect, as geometry and as area lights (sphere: cone sampling),
    in packet mode (records in constant memory) and through the BVH (k = analytic leaf records).  The quadrics are solved in double
    precision on both sides and the cylinder / cone / sphere maps use the shared polynomial sin/cos, so everything that does not touch the
    rough-conductor sphere is bit-exact against the oracle."""
    if bvh:
        monkeypatch.setenv("MI355PT_NO_PACKET", "1")
    sc = golden_scenes[name]; gs = mi.Scene(sc); orc = oracle.Oracle(sc); r = mi.Render(gs)
    nt, ns = len(sc.idx), len(sc.shapes)
    # closest hit / any hit for random rays
    rng = np.random.default_rng(77); n = 3000
    lo = np.array([min(sc.pos[:, k].min(), -6.0 if name == "shape_lights" else 0.0) for k in range(3)], np.float32); hi = -lo if name == "shape_lights" else sc.pos.max(0)
    o = (lo + rng.random((n, 3)) * (hi - lo)).astype(np.float32)
    d = rng.normal(size=(n, 3)); d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    rays = np.concatenate([o, np.full((n, 1), 1e-4, np.float32), d, np.full((n, 1), np.inf, np.float32)], 1).astype(np.float32)
    rays[200:500, 7] = rng.random(300).astype(np.float32) * (4 if name == "shape_lights" else 300)
    got = gs.intersect(rays); occ = gs.intersect(rays, any_hit=True); kinds = set()
    for i in range(n):
        ok, h = orc.intersect(rays[i])
        assert ok == (got[i, 3] >= 0)
        if ok:
            assert (bits(got[i, :3]) == bits(np.array([h[0], h[13], h[14]], np.float32))).all()
            shape = int(h[19]); prim = sc.shapes[shape]["first_tri"] + int(h[18]) if shape < ns else nt + shape - ns
            assert int(got[i, 3]) == prim
            kinds.add(-1 if shape < ns else sc.analytic[shape - ns]["type"])
        assert orc.occluded(rays[i]) == (occ[i, 3] >= 0)
    assert kinds >= ({-1, 0, 2, 3} if name != "cbox_shapes" else {-1, 0, 1, 2, 3})
    # radiance samples: oracle (same arithmetic) and the reference's own Li
    gd = np.load(os.path.join(GOLDEN, name + "_samples.npz")); pairs = gd["pairs"]
    ref = orc.render_samples(pairs)["li"]; got = r.samples(pairs)
    if name == "shape_lights":
        assert (bits(got) == bits(ref)).all()
    else:
        err = np.abs(got - ref).max(1) / (np.abs(ref).max(1) + 1e-6)
        assert (err < 1e-4).mean() > 0.995 and np.median(err) < 1e-6 and bit_share(got, ref, "analytic_shapes " + name) > 0.9999
    err = np.abs(got - gd["li"]).max(1) / (np.abs(gd["li"]).max(1) + 1e-6)
    assert (err < 1e-4).mean() > 0.99 and (err < 5e-3).mean() > 0.998 and np.median(err) < 1e-6
    # whole film + the ray counters
    r.run(); film = r.read_film(0); st = r.stats(); ofilm, cnt = orc.render_image(threads=4)
    rel = np.linalg.norm(film[..., :3] - ofilm[..., :3]) / np.linalg.norm(ofilm[..., :3])
    if name == "shape_lights":
        assert np.allclose(film, ofilm, rtol=2e-6, atol=1e-7) and (st["rays"], st["shadow_rays"], st["path_length_sum"]) == tuple(int(c) for c in cnt)
    else:
        assert rel < 2e-3 and abs(st["rays"] - int(cnt[0])) / cnt[0] < 1e-3 and abs(st["shadow_rays"] - int(cnt[1])) / cnt[1] < 1e-3
    ref_film = np.load(os.path.join(GOLDEN, name + "_image.npz"))["film"]
    assert np.linalg.norm(film[..., :3] - ref_film[..., :3]) / np.linalg.norm(ref_film[..., :3]) < 3e-3


@pytest.mark.parametrize("name", ["cbox_lights", "cbox_collimated", "cbox_roughdiffuse", "cbox_roughdiffuse_strict_indep", "cbox_phong", "cbox_phong_strict_indep", "cbox_ward", "cbox_ward_strict_indep", "ward_room", "cbox_coating", "cbox_coating_strict_indep", "blend_room", "cbox_roughcoating", "open_constant", "open_constant_hide_indep"])
def test_scene_level_emitters(mi, oracle, golden_scenes, name):
    """SURVEY.md §8f-4 emitters: `point` + `spot` next to the area light (emitter selection, delta lights: MIS weight 1) and a `constant`
    environment + `directional` light (cosine-hemisphere / uniform-sphere sampling, pdfDirect from the previous vertex' reference normal)."""
    sc = golden_scenes[name]; gs = mi.Scene(sc); orc = oracle.Oracle(sc); r = mi.Render(gs)
    gd = np.load(os.path.join(GOLDEN, name + "_samples.npz")); pairs = gd["pairs"]
    rng = np.random.default_rng(5); n = 20000
    more = np.stack([rng.integers(0, sc.width, n), rng.integers(0, sc.height, n), rng.integers(0, sc.spp, n)], 1).astype(np.uint32)
    ref = orc.render_samples(more)["li"]; got = r.samples(more)
    err = np.abs(got - ref).max(1) / (np.abs(ref).max(1) + 1e-6)
    if name in ("cbox_lights", "cbox_collimated", "cbox_roughdiffuse", "cbox_roughdiffuse_strict_indep", "cbox_phong", "cbox_phong_strict_indep", "cbox_ward", "cbox_ward_strict_indep", "ward_room", "cbox_coating", "cbox_coating_strict_indep", "blend_room", "cbox_roughcoating"):
        # all-diffuse; the spot's transition zone calls acosf (glibc's on both sides since round 3): bit-exact.  cbox_collimated: a `collimated` beam sits in the
        # emitter-selection CDF and never returns a sample (collimated.cpp:129-133).  cbox_roughdiffuse: Oren-Nayar, acosf / tanf / sincos from the glibc restatements
        assert bit_share(got, ref, name) > 0.9999 and (err < 1e-5).mean() > 0.999
    else:
        assert (err < 1e-4).mean() > 0.995 and np.median(err) < 1e-6          # rough-conductor sphere: tolerance-pinned
    got = r.samples(pairs); err = np.abs(got - gd["li"]).max(1) / (np.abs(gd["li"]).max(1) + 1e-6)   # the reference's own Li
    assert (err < 2e-4).mean() > 0.998 and np.median(err) < 1e-6
    r.run(); film = r.read_film(0); st = r.stats(); ofilm, cnt = orc.render_image(threads=4)
    assert np.linalg.norm(film[..., :3] - ofilm[..., :3]) / np.linalg.norm(ofilm[..., :3]) < 1e-3
    assert abs(st["rays"] - int(cnt[0])) / cnt[0] < 1e-3 and abs(st["shadow_rays"] - int(cnt[1])) / cnt[1] < 1e-3
    ref_film = np.load(os.path.join(GOLDEN, name + "_image.npz"))["film"]
    assert np.linalg.norm(film[..., :3] - ref_film[..., :3]) / np.linalg.norm(ref_film[..., :3]) < 1e-3


@pytest.mark.parametrize("name", ["cbox_materials", "cbox_materials_strict_indep"])
def test_smooth_bsdfs(mi, oracle, golden_scenes, name):
    """SURVEY.md §8f-2 BSDFs: `dielectric` (delta reflection + refraction, eta tracking for Russian roulette, radiance scaling), smooth
    `conductor`, `plastic` (delta coat over a diffuse base, linear and nonlinear), `twosided(conductor)`.  None of them calls the math library
    (Fresnel terms are +, *, /, sqrt), so the GPU equals the oracle bit for bit; vs the reference within float rounding."""
    sc = golden_scenes[name]; gs = mi.Scene(sc); orc = oracle.Oracle(sc); r = mi.Render(gs)
    gd = np.load(os.path.join(GOLDEN, name + "_samples.npz"))
    rng = np.random.default_rng(8); n = 20000
    pairs = np.stack([rng.integers(0, sc.width, n), rng.integers(0, sc.height, n), rng.integers(0, sc.spp, n)], 1).astype(np.uint32)
    ref = orc.render_samples(pairs)["li"]; got = r.samples(pairs)
    assert (bits(got) == bits(ref)).all()
    got = r.samples(gd["pairs"]); err = np.abs(got - gd["li"]).max(1) / (np.abs(gd["li"]).max(1) + 1e-6)      # the reference's own Li
    assert (err < 2e-4).mean() > 0.995 and (np.abs(got - gd["li"]).max(1) < 1e-4 * (1 + np.abs(gd["li"]).max(1))).all()
    r.run(); film = r.read_film(0); st = r.stats(); ofilm, cnt = orc.render_image(threads=4)
    assert np.allclose(film, ofilm, rtol=2e-6, atol=1e-7) and (st["rays"], st["shadow_rays"], st["path_length_sum"]) == tuple(int(c) for c in cnt)
    ref_film = np.load(os.path.join(GOLDEN, name + "_image.npz"))["film"]
    assert np.linalg.norm(film[..., :3] - ref_film[..., :3]) / np.linalg.norm(ref_film[..., :3]) < 1e-4


def test_instances(mi, oracle, golden_scenes):
    """`shapegroup` + `instance`.  The scene-level BVH holds one leaf record per instance; entering it takes the ray to the
    group's object space and walks the group's BVH with the same LDS stack.  Closest / any hit, the instance index and the radiance of
    every path that does not touch the rough-conductor lids are bit-exact against the oracle."""
    name = "instanced_garden"; sc = golden_scenes[name]; gs = mi.Scene(sc); orc = oracle.Oracle(sc); r = mi.Render(gs)
    rng = np.random.default_rng(99); n = 4000
    o = np.stack([rng.uniform(-7, 7, n), rng.uniform(0.05, 5, n), rng.uniform(-7, 7, n)], 1).astype(np.float32)
    d = rng.normal(size=(n, 3)); d[:, 1] -= 0.5; d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    rays = np.concatenate([o, np.full((n, 1), 1e-4, np.float32), d, np.full((n, 1), np.inf, np.float32)], 1).astype(np.float32)
    rays[100:600, 7] = rng.random(500).astype(np.float32) * 6
    (got, inst), occ = gs.intersect(rays, with_instance=True), gs.intersect(rays, any_hit=True); n_inst = 0
    for i in range(n):
        ok, h = orc.intersect(rays[i])
        assert ok == (got[i, 3] >= 0)
        if ok:
            assert (bits(got[i, :3]) == bits(np.array([h[0], h[13], h[14]], np.float32))).all()
            shape = int(h[19]); assert int(got[i, 3]) == sc.shapes[shape]["first_tri"] + int(h[18]) and inst[i] == int(h[20])
            n_inst += h[20] >= 0
        assert orc.occluded(rays[i]) == (occ[i, 3] >= 0)
    assert n_inst > n // 20
    gd = np.load(os.path.join(GOLDEN, name + "_samples.npz"))
    pairs = np.stack([rng.integers(0, sc.width, 20000), rng.integers(0, sc.height, 20000), rng.integers(0, sc.spp, 20000)], 1).astype(np.uint32)
    ref = orc.render_samples(pairs)["li"]; got = r.samples(pairs)
    err = np.abs(got - ref).max(1) / (np.abs(ref).max(1) + 1e-6)
    assert bit_share(got, ref, "instances") > 0.9999 and (err < 1e-4).mean() > 0.995 and np.median(err) < 1e-6
    got = r.samples(gd["pairs"]); err = np.abs(got - gd["li"]).max(1) / (np.abs(gd["li"]).max(1) + 1e-6)      # the reference's own Li
    assert (err < 2e-4).mean() > 0.99 and np.median(err) < 1e-6
    r.run(); film = r.read_film(0); st = r.stats(); ofilm, cnt = orc.render_image(threads=4)
    assert np.linalg.norm(film[..., :3] - ofilm[..., :3]) / np.linalg.norm(ofilm[..., :3]) < 2e-3
    assert abs(st["rays"] - int(cnt[0])) / cnt[0] < 1e-3 and abs(st["shadow_rays"] - int(cnt[1])) / cnt[1] < 1e-3
    ref_film = np.load(os.path.join(GOLDEN, name + "_image.npz"))["film"]
    assert np.linalg.norm(film[..., :3] - ref_film[..., :3]) / np.linalg.norm(ref_film[..., :3]) < 3e-3


@pytest.mark.parametrize("name", ["cbox_translucent", "cbox_translucent_indep"])
def test_rough_dielectric_and_difftrans(mi, oracle, golden_scenes, name):
    """`roughdielectric` (microfacet reflection / refraction with visible-normal sampling; draws one more sampler dimension per bounce, which
    shifts every later dimension of the path) and `difftrans`.  Microfacet code calls the math library -> tolerance-pinned like roughconductor."""
    sc = golden_scenes[name]; gs = mi.Scene(sc); orc = oracle.Oracle(sc); r = mi.Render(gs)
    gd = np.load(os.path.join(GOLDEN, name + "_samples.npz"))
    rng = np.random.default_rng(18); n = 20000
    pairs = np.stack([rng.integers(0, sc.width, n), rng.integers(0, sc.height, n), rng.integers(0, sc.spp, n)], 1).astype(np.uint32)
    ref = orc.render_samples(pairs)["li"]; got = r.samples(pairs)
    err = np.abs(got - ref).max(1) / (np.abs(ref).max(1) + 1e-6)
    assert (err < 1e-4).mean() > 0.99 and np.median(err) < 1e-6 and (bits(got) == bits(ref)).all(1).mean() > 0.5
    got = r.samples(gd["pairs"]); err = np.abs(got - gd["li"]).max(1) / (np.abs(gd["li"]).max(1) + 1e-6)      # the reference's own Li
    assert (err < 2e-4).mean() > 0.99 and np.median(err) < 1e-6
    r.run(); film = r.read_film(0); st = r.stats(); ofilm, cnt = orc.render_image(threads=4)
    assert np.linalg.norm(film[..., :3] - ofilm[..., :3]) / np.linalg.norm(ofilm[..., :3]) < 2e-3
    assert abs(st["rays"] - int(cnt[0])) / cnt[0] < 1e-3 and abs(st["shadow_rays"] - int(cnt[1])) / cnt[1] < 1e-3
    ref_film = np.load(os.path.join(GOLDEN, name + "_image.npz"))["film"]
    assert np.linalg.norm(film[..., :3] - ref_film[..., :3]) / np.linalg.norm(ref_film[..., :3]) < 2e-3


@pytest.mark.parametrize("name", ["cbox_roughplastic", "cbox_roughplastic_allnormals", "cbox_roughplastic_phong"])
def test_roughplastic(mi, oracle, golden_scenes, name):
    """`roughplastic`: glossy microfacet coat over a diffuse base; the rough-transmittance slice (100 values, Catmull-Rom lookup over the warped
    incidence angle) is material input data taken from the reference's own tables.  Microfacet code + powf -> tolerance-pinned.  The second scene
    samples all normals instead of the visible ones (sampleVisible = false)."""
    sc = golden_scenes[name]; gs = mi.Scene(sc); orc = oracle.Oracle(sc); r = mi.Render(gs)
    gd = np.load(os.path.join(GOLDEN, name + "_samples.npz"))
    rng = np.random.default_rng(28); n = 20000
    pairs = np.stack([rng.integers(0, sc.width, n), rng.integers(0, sc.height, n), rng.integers(0, sc.spp, n)], 1).astype(np.uint32)
    ref = orc.render_samples(pairs)["li"]; got = r.samples(pairs)
    err = np.abs(got - ref).max(1) / (np.abs(ref).max(1) + 1e-6)
    assert (err < 1e-4).mean() > 0.99 and np.median(err) < 1e-6
    got = r.samples(gd["pairs"]); err = np.abs(got - gd["li"]).max(1) / (np.abs(gd["li"]).max(1) + 1e-6)      # the reference's own Li
    assert (err < 2e-4).mean() > 0.99 and np.median(err) < 1e-6
    r.run(); film = r.read_film(0); st = r.stats(); ofilm, cnt = orc.render_image(threads=4)
    assert np.linalg.norm(film[..., :3] - ofilm[..., :3]) / np.linalg.norm(ofilm[..., :3]) < 2e-3
    assert abs(st["rays"] - int(cnt[0])) / cnt[0] < 1e-3 and abs(st["shadow_rays"] - int(cnt[1])) / cnt[1] < 1e-3
    ref_film = np.load(os.path.join(GOLDEN, name + "_image.npz"))["film"]
    assert np.linalg.norm(film[..., :3] - ref_film[..., :3]) / np.linalg.norm(ref_film[..., :3]) < 2e-3
    with pytest.raises(mi.MiError, match="rough-transmittance"):
        bad = mi.scenes.cbox_roughplastic(32, 32, 1); bad.material_tables = None; mi.Scene(bad)


def test_texture_coordinates_and_procedural_textures(mi, oracle, golden_scenes):
    """Meshes with texture coordinates: its.uv interpolation and shading frames from the UV tangents (TriMesh::computeUVTangents), `checkerboard`
    and `gridtexture` bound to diffuse reflectances (no filtering in the reference either).  All-diffuse -> bit-exact against the oracle."""
    name = "textured_room"; sc = golden_scenes[name]; gs = mi.Scene(sc); orc = oracle.Oracle(sc); r = mi.Render(gs)
    gd = np.load(os.path.join(GOLDEN, name + "_samples.npz"))
    rng = np.random.default_rng(38); n = 20000
    pairs = np.stack([rng.integers(0, sc.width, n), rng.integers(0, sc.height, n), rng.integers(0, sc.spp, n)], 1).astype(np.uint32)
    ref = orc.render_samples(pairs)["li"]; got = r.samples(pairs)
    assert (bits(got) == bits(ref)).all()
    got = r.samples(gd["pairs"]); err = np.abs(got - gd["li"]).max(1) / (np.abs(gd["li"]).max(1) + 1e-6)      # the reference's own Li
    assert (err < 2e-4).mean() > 0.998 and np.median(err) < 1e-6
    r.run(); film = r.read_film(0); st = r.stats(); ofilm, cnt = orc.render_image(threads=4)
    assert np.allclose(film, ofilm, rtol=2e-6, atol=1e-7) and (st["rays"], st["shadow_rays"], st["path_length_sum"]) == tuple(int(c) for c in cnt)
    ref_film = np.load(os.path.join(GOLDEN, name + "_image.npz"))["film"]
    assert np.linalg.norm(film[..., :3] - ref_film[..., :3]) / np.linalg.norm(ref_film[..., :3]) < 5e-4


def test_bitmap_textures(mi, oracle, golden_scenes):
    """`bitmap` textures: MIP pyramid as input data, EWA (anisotropic footprints on the floor, clamped anisotropy), trilinear, bilinear and
    nearest lookups, repeat / mirror / clamp / zero / one wrapping; the camera hit filters with Intersection::computePartials, later bounces read
    level 0.  log / atan / sin / cos of the level selection are glibc's routines restated on the device (csrc/libm_glibc.h): bit share >= 0.9999 (measured 1.0000)."""
    name = "bitmap_room"; sc = golden_scenes[name]; gs = mi.Scene(sc); orc = oracle.Oracle(sc); r = mi.Render(gs)
    gd = np.load(os.path.join(GOLDEN, name + "_samples.npz"))
    rng = np.random.default_rng(48); n = 20000
    pairs = np.stack([rng.integers(0, sc.width, n), rng.integers(0, sc.height, n), rng.integers(0, sc.spp, n)], 1).astype(np.uint32)
    ref = orc.render_samples(pairs)["li"]; got = r.samples(pairs)
    err = np.abs(got - ref).max(1) / (np.abs(ref).max(1) + 1e-6)
    assert (err < 1e-4).mean() > 0.998 and np.median(err) < 1e-6 and bit_share(got, ref, "bitmap_textures") >= 0.9999
    got = r.samples(gd["pairs"]); err = np.abs(got - gd["li"]).max(1) / (np.abs(gd["li"]).max(1) + 1e-6)      # the reference's own Li
    assert (err < 2e-4).mean() > 0.998 and np.median(err) < 1e-6
    r.run(); film = r.read_film(0); st = r.stats(); ofilm, cnt = orc.render_image(threads=4)
    assert np.linalg.norm(film[..., :3] - ofilm[..., :3]) / np.linalg.norm(ofilm[..., :3]) < 5e-4
    assert (st["rays"], st["shadow_rays"], st["path_length_sum"]) == tuple(int(c) for c in cnt)
    ref_film = np.load(os.path.join(GOLDEN, name + "_image.npz"))["film"]
    assert np.linalg.norm(film[..., :3] - ref_film[..., :3]) / np.linalg.norm(ref_film[..., :3]) < 5e-4
    with pytest.raises(mi.MiError, match="MIP levels"):
        bad = mi.scenes.bitmap_room(32, 32, 1); bad.texture_levels = None; mi.Scene(bad)


@pytest.mark.parametrize("config", ["C3_veach_1080p", "C4_atrium_4k"])
def test_full_size_other_configs(mi, config):
    """BASELINE configs 3 and 4 at their full film sizes (fewer sample planes than quoted, the planes are independent): properties that need no
    CPU oracle -- finite non-negative film, weight channel = spp, additivity over sample ranges and interleaved rows, ray counters in range."""
    S = mi.scenes
    if config == "C3_veach_1080p":
        sc = S.veach_mis(1920, 1080, 512, max_depth=12); spp = 8; lo, hi = 2.0, 4.5
    else:
        sc = S.atrium(3840, 2160, 64); spp = 4; lo, hi = 3.0, 7.0
    gs = mi.Scene(sc); r = mi.Render(gs)
    r.run(s0=0, s1=spp); full = r.read_film(0); st = r.stats(); n = sc.width * sc.height * spp
    assert st["samples"] == n and lo < st["rays"] / n < hi
    assert np.isfinite(full).all() and (full >= 0).all()
    w = full[1:-1, 1:-1, 4]; w0 = np.median(w); assert abs(w0 / spp - 1) < 1e-3 and np.isclose(w, w0, rtol=1e-3).mean() > 0.98
    r.clear(); r.run(s0=0, s1=spp // 2); r.run(s0=spp // 2, s1=spp); parts = r.read_film(0)
    assert np.allclose(parts, full, rtol=1e-5, atol=1e-6)
    r.clear()
    for k in range(2):
        r.run(tile=(0, k, sc.width, sc.height), s0=0, s1=spp, row_stride=2)
    inter = r.read_film(0)
    assert np.allclose(inter, full, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("config", ["C2_cornell_1080p_256spp", "C3_veach_1080p_512spp", "C4_atrium_4k_64spp"])
def test_full_size_configs_spot_check_vs_oracle(mi, oracle, config):
    """The BASELINE configurations at their FULL film size and sample count, spot-checked against the oracle: random (pixel, sample index) pairs over the
    whole range (Sobol indices up to 512 planes at 1080p / 64 at 4K, the 251 k-triangle BVH).  Cornell: bit-exact; Veach (rough conductors) and the atrium
    (environment map, smooth-shaded columns) within the tolerance of their small-film tests."""
    S = mi.scenes
    sc = {"C2": lambda: S.cornell_box(1920, 1080, 256), "C3": lambda: S.veach_mis(1920, 1080, 512, max_depth=12), "C4": lambda: S.atrium(3840, 2160, 64)}[config[:2]]()
    gs = mi.Scene(sc); r = mi.Render(gs); orc = oracle.Oracle(sc)
    rng = np.random.default_rng(2025); n = 6000
    pairs = np.stack([rng.integers(0, sc.width, n), rng.integers(0, sc.height, n), rng.integers(0, sc.spp, n)], 1).astype(np.uint32)
    pairs[:4] = [[0, 0, 0], [sc.width - 1, sc.height - 1, sc.spp - 1], [sc.width - 1, 0, sc.spp // 2], [0, sc.height - 1, 1]]
    ref = orc.render_samples(pairs)["li"]; got = r.samples(pairs)
    if config.startswith("C2"):
        assert (bits(got) == bits(ref)).all()
    else:
        err = np.abs(got - ref).max(1) / (np.abs(ref).max(1) + 1e-6)
        assert (err < 1e-4).mean() > 0.99 and (err < 1e-2).mean() > 0.998 and np.median(err) < 1e-6, ((err < 1e-4).mean(), (err < 1e-2).mean())
        assert bit_share(got, ref, "full_size " + config) > 0.9999      # Veach (rough conductors) and the atrium (environment map) at full size: bit-exact as well
    assert np.isfinite(got).all() and (got >= 0).all() and got.max() > 0


def test_config5_rows_of_eight_ranks_on_one_gpu(mi, oracle):
    """BASELINE config 5 (the 4K atrium at 1024 spp, film rows interleaved over 8 GPUs) as far as ONE GPU can show it: 35-bit Sobol indices on the 251 k-triangle
    scene, every row class k = y mod 8 spot-checked against the oracle with sample indices from the whole range [0, 1024), and the eight rank shares
    (mi_render_run_rows, stride 8, two high sample planes) summing to the unsplit film.  What is NOT shown here: eight devices, RCCL, xGMI (no such node in the loop)."""
    S = mi.scenes
    sc = S.atrium(3840, 2160, 1024); gs = mi.Scene(sc); r = mi.Render(gs); orc = oracle.Oracle(sc)
    rng = np.random.default_rng(55); n = 4800
    pairs = np.stack([rng.integers(0, sc.width, n), rng.integers(0, sc.height, n), rng.integers(0, 1024, n)], 1).astype(np.uint32)
    pairs[:, 1] = (pairs[:, 1] // 8) * 8 + (np.arange(n) % 8)                  # 600 samples per row class
    pairs[:3] = [[0, 0, 1023], [sc.width - 1, sc.height - 1, 1023], [sc.width // 2, 7, 512]]
    ref = orc.render_samples(pairs)["li"]; got = r.samples(pairs)
    err = np.abs(got - ref).max(1) / (np.abs(ref).max(1) + 1e-6)
    assert bit_share(got, ref, "config5") > 0.9999
    for k in range(8):
        sel = (pairs[:, 1] % 8) == k
        assert sel.sum() >= 590 and (err[sel] < 1e-4).mean() > 0.985 and np.median(err[sel]) < 1e-6, (k, (err[sel] < 1e-4).mean())
    assert np.isfinite(got).all() and (got >= 0).all() and got.max() > 0
    r.clear(); r.run(s0=1000, s1=1002); full = r.read_film(0); rays_full = r.stats()["rays"]
    acc = np.zeros_like(full); rays = 0
    for k in range(8):
        r.clear(); r.run(tile=(0, k, sc.width, sc.height), s0=1000, s1=1002, row_stride=8); part = r.read_film(0); rays += r.stats()["rays"]
        b = r.film_shape(0)[3]; pin = part[b:part.shape[0] - b, b:part.shape[1] - b]; fin = full[b:full.shape[0] - b, b:full.shape[1] - b]      # (the film carries the filter's border)
        other = np.delete(pin[..., 4], np.s_[k::8], axis=0)
        assert (bits(pin[k::8]) == bits(fin[k::8])).all(2).mean() > 0.999 and (other == 0.0).mean() > 0.9999      # own rows: the unsplit film's; other ranks' rows untouched (edge splats of the box filter aside)
        acc += part
    assert rays == rays_full
    same = (bits(acc) == bits(full)).all(2)
    assert same.mean() > 0.9999 and np.allclose(acc, full, rtol=1e-6, atol=1e-7)


def test_scene_file_bunny(mi, oracle, golden_scenes, tmp_path):
    """a scene FILE (tests/golden/meshes/bunny_box.xml: hand-written Mitsuba XML around the reference's own PLY test asset) read by
    xml_scene / meshio and rendered by the HIP path: bit-exact against the oracle (diffuse + smooth dielectric, generated vertex normals on 69451
    triangles -> BVH2 traversal), within float rounding of the reference's own render of the same flattened scene; then through the command line."""
    import importlib
    name = "bunny_box"; sc = golden_scenes[name]; gs = mi.Scene(sc); orc = oracle.Oracle(sc); r = mi.Render(gs)
    rng = np.random.default_rng(5); n = 20000
    pairs = np.stack([rng.integers(0, sc.width, n), rng.integers(0, sc.height, n), rng.integers(0, sc.spp, n)], 1).astype(np.uint32)
    ref = orc.render_samples(pairs)["li"]; got = r.samples(pairs)
    assert (bits(got) == bits(ref)).all()
    gd = np.load(os.path.join(GOLDEN, name + "_samples.npz"))
    got = r.samples(gd["pairs"]); err = np.abs(got - gd["li"]).max(1) / (np.abs(gd["li"]).max(1) + 1e-6)
    assert (err < 2e-4).mean() > 0.99 and np.median(err) < 1e-6
    r.run(); film = r.read_film(0); st = r.stats(); ofilm, cnt = orc.render_image(threads=4)
    assert np.allclose(film, ofilm, rtol=2e-6, atol=1e-7) and (st["rays"], st["shadow_rays"], st["path_length_sum"]) == tuple(int(c) for c in cnt)
    ref_film = np.load(os.path.join(GOLDEN, name + "_image.npz"))["film"]
    assert np.linalg.norm(film[..., :3] - ref_film[..., :3]) / np.linalg.norm(ref_film[..., :3]) < 1e-3
    # the command-line front end renders the same image (developed film = sums / weights)
    render_cli = importlib.import_module("mitsuba-im_amd.render")
    out = str(tmp_path / "bunny.npy")
    assert render_cli.main([os.path.join(GOLDEN, "meshes", "bunny_box.xml"), "-o", out]) == 0
    b = (film.shape[0] - sc.height) // 2
    dev = film[b:b + sc.height, b:b + sc.width, :3] / film[b:b + sc.height, b:b + sc.width, 4:5]
    np.testing.assert_allclose(np.load(out), dev, rtol=1e-6, atol=1e-7)
    assert render_cli.main([str(tmp_path / "missing.xml")]) == 1


def test_scene_file_with_exr_environment(mi, oracle, tmp_path):
    """Scene ingestion incl. image decoding: tests/golden/scenes/sky_ball.xml lights a ball with the reference's own PIZ-compressed OpenEXR test asset
    (imageio.py); the HIP path agrees with the oracle on the scene as loaded, and the CLI writes the developed film as OpenEXR / PNG."""
    import importlib
    xml_scene = importlib.import_module("mitsuba-im_amd.xml_scene"); imageio = importlib.import_module("mitsuba-im_amd.imageio")
    path = os.path.join(GOLDEN, "scenes", "sky_ball.xml")
    sc = xml_scene.load_scene(path)
    assert sc.envmap["rgb"].shape == (256, 512, 3)
    gs = mi.Scene(sc); orc = oracle.Oracle(sc); r = mi.Render(gs)
    r.run(); film = r.read_film(0); st = r.stats(); ofilm, cnt = orc.render_image(threads=4)
    err = np.abs(film - ofilm).max(-1) / (np.abs(ofilm).max(-1) + 1e-6)
    assert (err < 1e-4).mean() > 0.995 and np.median(err) < 1e-6                        # libm in the microfacet / lat-long code
    rel = np.linalg.norm(film[..., :3] - ofilm[..., :3]) / np.linalg.norm(ofilm[..., :3])
    assert rel < 1e-4 and abs(st["rays"] - int(cnt[0])) <= 4
    render_cli = importlib.import_module("mitsuba-im_amd.render")
    out = str(tmp_path / "sky.exr")
    assert render_cli.main([path, "-o", out]) == 0
    b = (film.shape[0] - sc.height) // 2
    dev = film[b:b + sc.height, b:b + sc.width, :3] / film[b:b + sc.height, b:b + sc.width, 4:5]
    px, names = imageio.read_exr(out)
    np.testing.assert_allclose(imageio._exr_planes(px, names), dev, rtol=1e-6, atol=1e-7)
    assert dev[:10].mean() > 0.05 and np.isfinite(dev).all()                            # the sky is visible behind the ball
    png = str(tmp_path / "sky.png")
    assert render_cli.main([path, "-o", png, "--spp", "2"]) == 0 and os.path.getsize(png) > 500


def test_scene_file_round_trip_renders_identically(mi, tmp_path):
    """export_scene -> load_scene: the HIP path renders the same film from the scene file as from the generator (Cornell box, serialized meshes)."""
    import importlib
    X = importlib.import_module("mitsuba-im_amd.xml_scene"); S = mi.scenes
    sc = S.cornell_box(width=160, height=90, spp=8)
    sc.xfov = float(np.float32(sc.xfov)); sc.sample_to_camera = S.sample_to_camera(sc.xfov, sc.near, sc.far, sc.width / sc.height)
    sc2 = X.load_scene(X.export_scene(sc, str(tmp_path)))
    films = []
    for s in (sc, sc2):
        r = mi.Render(mi.Scene(s)); r.run(); films.append(r.read_film(0))
    assert (bits(films[0]) == bits(films[1])).all()


@pytest.mark.parametrize("name", ["sky_view", "sky_view_indep"])
def test_filtered_environment_lookups(mi, oracle, golden_scenes, name):
    """SURVEY.md §8 a10, camera rays: EnvironmentMap::evalEnvironment with the sensor ray's differentials (texture-space partials -> TMIPMap::eval, EWA with
    anisotropy <= 10 over the map's MIP pyramid; `k_env_primary` between the first extend and the first shade).  The pyramid is built by
    scenes.build_mip_pyramid (pinned against the reference's Bitmap::resample).  log / atan / sin / cos of the level and ellipse selection come from the
    device math library -> tolerance-pinned against the oracle; the reference's own samples and film next to it."""
    sc = golden_scenes[name]; gs = mi.Scene(sc); orc = oracle.Oracle(sc); r = mi.Render(gs)
    gd = np.load(os.path.join(GOLDEN, name + "_samples.npz"))
    ref = orc.render_samples(gd["pairs"])["li"]; got = r.samples(gd["pairs"])
    err = np.abs(got - ref).max(1) / (np.abs(ref).max(1) + 1e-6)
    assert (err < 1e-5).mean() > 0.95 and (err < 1e-3).mean() > 0.995 and err.max() < 5e-3, ((err < 1e-5).mean(), err.max())     # a last-bit change of the ellipse coefficients moves a texel in or out of the EWA footprint
    err = np.abs(got - gd["li"]).max(1) / (np.abs(gd["li"]).max(1) + 1e-6)                    # the reference's own Li
    assert (err < 1e-4).mean() > 0.98 and err.max() < 5e-3 and np.median(err) < 1e-6
    r.run(); film = r.read_film(0); ofilm, cnt = orc.render_image(threads=4); st = r.stats()
    assert np.linalg.norm(film[..., :3] - ofilm[..., :3]) / np.linalg.norm(ofilm[..., :3]) < 2e-4
    assert (st["rays"], st["shadow_rays"]) == (int(cnt[0]), int(cnt[1]))
    ref_film = np.load(os.path.join(GOLDEN, name + "_image.npz"))["film"]
    assert np.linalg.norm(film[..., :3] - ref_film[..., :3]) / np.linalg.norm(ref_film[..., :3]) < 2e-4
    # without the pyramid (mi_scene_set_envmap_filter not called) the camera-ray samples are the level-0 lookups: far from the reference here
    sc0 = type(sc)(sc); sc0["env_texture"] = 0
    r0 = mi.Render(mi.Scene(sc0)); r0.run(); f0 = r0.read_film(0)
    assert np.linalg.norm(f0[..., :3] - ref_film[..., :3]) / np.linalg.norm(ref_film[..., :3]) > 5e-2
    # hideEmitters: camera rays do not see the map at all (path.cpp:139), with or without the pyramid
    rh = mi.Render(gs, hide_emitters=True); rh.run(); fh = rh.read_film(0)
    oh = type(sc)(sc); oh["hide_emitters"] = 1; ofh, _ = oracle.Oracle(oh).render_image(threads=4)
    assert np.linalg.norm(fh[..., :3] - ofh[..., :3]) / max(np.linalg.norm(ofh[..., :3]), 1e-9) < 1e-4


def test_sobol_scramble(mi, oracle, golden_scenes):
    """SobolSampler `scramble` != 0 (src/samplers/sobol.cpp:92-102, sobolseq.h:43-58, :99-131): the value goes through sampleTEA on the host, is XORed into
    every sample and flips the pixel bits of look_up -- integer math, bit-exact against the oracle; the reference's own samples next to it."""
    name = "cornell_scramble"; sc = golden_scenes[name]; gs = mi.Scene(sc); orc = oracle.Oracle(sc); r = mi.Render(gs)
    gd = np.load(os.path.join(GOLDEN, name + "_samples.npz"))
    rng = np.random.default_rng(12); n = 20000
    pairs = np.stack([rng.integers(0, sc.width, n), rng.integers(0, sc.height, n), rng.integers(0, sc.spp, n)], 1).astype(np.uint32)
    assert (bits(r.samples(pairs)) == bits(orc.render_samples(pairs)["li"])).all()
    got = r.samples(gd["pairs"]); err = np.abs(got - gd["li"]).max(1) / (np.abs(gd["li"]).max(1) + 1e-6)
    assert (err < 2e-4).mean() > 0.998 and err.max() < 5e-3
    r.run(); film = r.read_film(0); ofilm, _ = orc.render_image(threads=4)
    assert (bits(film) == bits(ofilm)).all()
    r0 = mi.Render(gs, seed=0); r0.run()
    assert not np.array_equal(r0.read_film(0), film)                 # a different scramble is a different sequence ...
    ref_film = np.load(os.path.join(GOLDEN, name + "_image.npz"))["film"]
    assert np.linalg.norm(film[..., :3] - ref_film[..., :3]) / np.linalg.norm(ref_film[..., :3]) < 1e-4       # ... and this one is the reference's


@pytest.mark.parametrize("name", ["veach_microfacets", "veach_microfacets_2", "cbox_translucent_mf", "cbox_translucent_mf2"])
def test_full_microfacet_distribution(mi, oracle, golden_scenes, name):
    """SURVEY.md §8 a12, the rest of MicrofacetDistribution under roughconductor (src/bsdfs/microfacet.h): anisotropic Beckmann / GGX (alphaU != alphaV, the
    tangent comes from the plates' texture coordinates), sampleVisible = false (sampleAll / pdfAll and the D G (wi.m) / (pdf cos) weight), Phong and
    Ashikhmin-Shirley; and under roughdielectric (cbox_translucent_mf*: anisotropic sphere, Walter's widened sampling distribution for all-normal sampling,
    Phong slab; roughdielectric.cpp:409-414, 607-612).  exp / log / pow / atan / tan come from the device math library -> tolerance-pinned against the oracle, the reference's own samples
    and film next to it."""
    sc = golden_scenes[name]; gs = mi.Scene(sc); orc = oracle.Oracle(sc); r = mi.Render(gs)
    gd = np.load(os.path.join(GOLDEN, name + "_samples.npz"))
    rng = np.random.default_rng(21); n = 20000
    pairs = np.stack([rng.integers(0, sc.width, n), rng.integers(0, sc.height, n), rng.integers(0, sc.spp, n)], 1).astype(np.uint32)
    ref = orc.render_samples(pairs)["li"]; got = r.samples(pairs)
    err = np.abs(got - ref).max(1) / (np.abs(ref).max(1) + 1e-6)
    assert (err < 1e-4).mean() > 0.99 and (err < 1e-2).mean() > 0.999 and np.median(err) < 1e-6, ((err < 1e-4).mean(), (err < 1e-2).mean(), np.median(err))
    got = r.samples(gd["pairs"]); err = np.abs(got - gd["li"]).max(1) / (np.abs(gd["li"]).max(1) + 1e-6)      # the reference's own Li
    assert (err < 1e-3).mean() > 0.99 and np.median(err) < 1e-6
    r.run(); film = r.read_film(0); ofilm, cnt = orc.render_image(threads=4); st = r.stats()
    assert np.linalg.norm(film[..., :3] - ofilm[..., :3]) / np.linalg.norm(ofilm[..., :3]) < 2e-3
    assert abs(st["rays"] - int(cnt[0])) / cnt[0] < 1e-3
    ref_film = np.load(os.path.join(GOLDEN, name + "_image.npz"))["film"]
    assert np.linalg.norm(film[..., :3] - ref_film[..., :3]) / np.linalg.norm(ref_film[..., :3]) < 2e-3
    # an anisotropic material on a mesh without texture coordinates is refused like TriMesh::computeUVTangents does
    bad = type(sc)(sc); bad["shapes"] = [dict(s, has_uv=0) for s in sc.shapes]
    if any(sc.bsdfs[s["bsdf"]].get("aniso") for s in sc.shapes):      # (analytic shapes carry their own parameterisation)
        with pytest.raises(mi.MiError, match="texture coordinates are required"):
            mi.Scene(bad)


def test_textures_on_plastic_and_difftrans(mi, oracle, golden_scenes):
    """textures on plastic.diffuseReflectance (checkerboard, nonlinear), roughplastic.diffuseReflectance (bitmap, trilinear; grid) and
    difftrans.transmittance (grid).  The lobe-selection weight comes from the texture's AVERAGE (plastic.cpp:204-207; derived on the host at commit), the
    lobes use the local value.  Procedural textures and the smooth plastic are libm-free -> most samples bit-exact; roughplastic / bitmap level selection
    are tolerance-pinned."""
    name = "textured_plastics"; sc = golden_scenes[name]; gs = mi.Scene(sc); orc = oracle.Oracle(sc); r = mi.Render(gs)
    gd = np.load(os.path.join(GOLDEN, name + "_samples.npz"))
    rng = np.random.default_rng(77); n = 20000
    pairs = np.stack([rng.integers(0, sc.width, n), rng.integers(0, sc.height, n), rng.integers(0, sc.spp, n)], 1).astype(np.uint32)
    ref = orc.render_samples(pairs)["li"]; got = r.samples(pairs)
    err = np.abs(got - ref).max(1) / (np.abs(ref).max(1) + 1e-6)
    assert (err < 1e-5).mean() > 0.99 and (err < 1e-2).mean() > 0.999 and np.median(err) < 1e-6, ((err < 1e-5).mean(), err.max())
    got = r.samples(gd["pairs"]); err = np.abs(got - gd["li"]).max(1) / (np.abs(gd["li"]).max(1) + 1e-6)      # the reference's own Li
    assert (err < 1e-4).mean() > 0.995 and np.median(err) < 1e-6
    r.run(); film = r.read_film(0); ofilm, cnt = orc.render_image(threads=4); st = r.stats()
    assert np.linalg.norm(film[..., :3] - ofilm[..., :3]) / np.linalg.norm(ofilm[..., :3]) < 1e-3
    assert abs(st["rays"] - int(cnt[0])) / cnt[0] < 1e-3
    ref_film = np.load(os.path.join(GOLDEN, name + "_image.npz"))["film"]
    assert np.linalg.norm(film[..., :3] - ref_film[..., :3]) / np.linalg.norm(ref_film[..., :3]) < 1e-3
    # a texture on a parameter the path takes as a constant only is refused
    bad = type(sc)(sc); bad["bsdfs"] = [dict(b) for b in sc.bsdfs]; bad["bsdfs"][4] = dict(mi.scenes.make_bsdf(kind=mi.scenes.BSDF_CONDUCTOR), texture=0)
    with pytest.raises(mi.MiError, match="textures bind to"):
        mi.Scene(bad)


@pytest.mark.parametrize("name", ["glass_pane", "glass_pane_hide_indep"])
def test_thin_dielectric(mi, oracle, golden_scenes, name):
    """`thindielectric` (src/bsdfs/thindielectric.cpp) -- delta reflection or straight-through transmission with the pane's internal bounces
    summed.  The transmission is an ENull component: a path that has only crossed panes is still "unscattered" (path.cpp:213), which with hideEmitters keeps
    the sky hidden through the glass (:238-239) but not the area light (:226-231); carried as one state bit.  No math library calls -> bit-exact."""
    sc = golden_scenes[name]; gs = mi.Scene(sc); orc = oracle.Oracle(sc); r = mi.Render(gs)
    gd = np.load(os.path.join(GOLDEN, name + "_samples.npz"))
    rng = np.random.default_rng(4); n = 20000
    pairs = np.stack([rng.integers(0, sc.width, n), rng.integers(0, sc.height, n), rng.integers(0, sc.spp, n)], 1).astype(np.uint32)
    ref = orc.render_samples(pairs)["li"]; got = r.samples(pairs)
    err = np.abs(got - ref).max(1) / (np.abs(ref).max(1) + 1e-6)          # the gold sphere's rough conductor goes through the device math library
    assert bit_share(got, ref, "thin_dielectric " + name) > 0.9999 and (err < 1e-4).mean() > 0.995 and np.median(err) == 0
    got = r.samples(gd["pairs"]); err = np.abs(got - gd["li"]).max(1) / (np.abs(gd["li"]).max(1) + 1e-6)      # the reference's own Li
    assert (err < 1e-4).mean() > 0.995 and np.median(err) < 1e-6
    r.run(); film = r.read_film(0); ofilm, cnt = orc.render_image(threads=4); st = r.stats()
    assert np.linalg.norm(film[..., :3] - ofilm[..., :3]) / np.linalg.norm(ofilm[..., :3]) < 1e-4
    assert abs(st["rays"] - int(cnt[0])) / cnt[0] < 1e-3
    ref_film = np.load(os.path.join(GOLDEN, name + "_image.npz"))["film"]
    assert np.linalg.norm(film[..., :3] - ref_film[..., :3]) / np.linalg.norm(ref_film[..., :3]) < 1e-4
    # hideEmitters changes what is seen THROUGH the pane: the sky disappears there too
    other = mi.Render(gs, hide_emitters=not sc.hide_emitters); other.run()
    assert np.linalg.norm(other.read_film(0)[..., :3] - film[..., :3]) / np.linalg.norm(film[..., :3]) > 0.05


@pytest.mark.parametrize("name", ["masked_room", "masked_room_hide_indep"])
def test_mask(mi, oracle, golden_scenes, name):
    """`mask` (src/bsdfs/mask.cpp) -- an opacity (checkerboard / grid texture, coloured constant) in front of a nested material record: eval and
    pdf scaled by opacity / its luminance, the nested BSDF or a straight pass-through (ENull: the path stays unscattered, hideEmitters keeps hiding the sky
    through the holes) chosen by sample.x, which is rescaled for the nested sampler.  Diffuse / plastic nested BSDFs are libm-free -> bit-exact; the grille's
    rough conductor is tolerance-pinned."""
    sc = golden_scenes[name]; gs = mi.Scene(sc); orc = oracle.Oracle(sc); r = mi.Render(gs)
    gd = np.load(os.path.join(GOLDEN, name + "_samples.npz"))
    rng = np.random.default_rng(14); n = 20000
    pairs = np.stack([rng.integers(0, sc.width, n), rng.integers(0, sc.height, n), rng.integers(0, sc.spp, n)], 1).astype(np.uint32)
    ref = orc.render_samples(pairs)["li"]; got = r.samples(pairs)
    err = np.abs(got - ref).max(1) / (np.abs(ref).max(1) + 1e-6)
    assert bit_share(got, ref, "mask " + name) > 0.9999 and (err < 1e-4).mean() > 0.995 and np.median(err) == 0
    got = r.samples(gd["pairs"]); err = np.abs(got - gd["li"]).max(1) / (np.abs(gd["li"]).max(1) + 1e-6)      # the reference's own Li
    assert (err < 1e-4).mean() > 0.995 and np.median(err) < 1e-6
    r.run(); film = r.read_film(0); ofilm, cnt = orc.render_image(threads=4); st = r.stats()
    assert np.linalg.norm(film[..., :3] - ofilm[..., :3]) / np.linalg.norm(ofilm[..., :3]) < 1e-4
    assert abs(st["rays"] - int(cnt[0])) / cnt[0] < 1e-3
    ref_film = np.load(os.path.join(GOLDEN, name + "_image.npz"))["film"]
    assert np.linalg.norm(film[..., :3] - ref_film[..., :3]) / np.linalg.norm(ref_film[..., :3]) < 1e-4
    # validation: a mask must point at an existing non-mask record
    bad = type(sc)(sc); bad["bsdfs"] = [dict(b) for b in sc.bsdfs]
    mi_ = [i for i, b in enumerate(sc.bsdfs) if b["type"] == mi.scenes.BSDF_MASK]
    bad["bsdfs"][mi_[0]]["distr"] = mi_[1]
    with pytest.raises(mi.MiError, match="nested material record"):
        mi.Scene(bad)


def test_textures_on_analytic_shapes(mi, oracle, golden_scenes):
    """Textures on analytic shapes through the shapes' own (u, v) parameterisations and tangents (rectangle.cpp:161-163, disk.cpp:173-193, sphere.cpp:218-245,
    cylinder.cpp:204-216), evaluated on demand in the texture block of k_shade: checkerboard rectangle floor, grid-textured plastic sphere, EWA-filtered bitmap on
    a cylinder (camera-hit footprints from the analytic dp/du, dp/dv), checkerboard disk, checkerboard-masked rectangle.  atan2 / acos of the parameterisations
    come from the device math library -> tolerance-pinned; the reference's own samples and film next to it."""
    name = "textured_shapes"; sc = golden_scenes[name]; gs = mi.Scene(sc); orc = oracle.Oracle(sc); r = mi.Render(gs)
    gd = np.load(os.path.join(GOLDEN, name + "_samples.npz"))
    rng = np.random.default_rng(41); n = 20000
    pairs = np.stack([rng.integers(0, sc.width, n), rng.integers(0, sc.height, n), rng.integers(0, sc.spp, n)], 1).astype(np.uint32)
    ref = orc.render_samples(pairs)["li"]; got = r.samples(pairs)
    err = np.abs(got - ref).max(1) / (np.abs(ref).max(1) + 1e-6)
    assert (err < 1e-5).mean() > 0.99 and (err < 1e-2).mean() > 0.998 and np.median(err) < 1e-6, ((err < 1e-5).mean(), (err < 1e-2).mean())
    got = r.samples(gd["pairs"]); err = np.abs(got - gd["li"]).max(1) / (np.abs(gd["li"]).max(1) + 1e-6)      # the reference's own Li
    assert (err < 1e-4).mean() > 0.99 and np.median(err) < 1e-6
    r.run(); film = r.read_film(0); ofilm, cnt = orc.render_image(threads=4); st = r.stats()
    assert np.linalg.norm(film[..., :3] - ofilm[..., :3]) / np.linalg.norm(ofilm[..., :3]) < 2e-3
    assert abs(st["rays"] - int(cnt[0])) / cnt[0] < 1e-3
    ref_film = np.load(os.path.join(GOLDEN, name + "_image.npz"))["film"]
    assert np.linalg.norm(film[..., :3] - ref_film[..., :3]) / np.linalg.norm(ref_film[..., :3]) < 2e-3


def test_sobol_dimension_budget_with_sampler_drawing_bsdfs(mi):
    """A rough dielectric draws one more sampler value per bounce (EUsesSampler): the Sobol dimension budget and the staged lookup tables count 6 per bounce
    then, so the reference's "Lookup dimension exceeds the direction number table size" arrives before a path could read past the tables."""
    S = mi.scenes
    gs = mi.Scene(S.cbox_translucent(width=32, height=32, spp=2, max_depth=20))
    mi.Render(gs).run()                                             # 3 + 6 * 20 = 123 <= 128 loaded dimensions
    with pytest.raises(mi.MiError, match="Lookup dimension exceeds"):
        mi.Render(gs, max_depth=21)                                 # 129 > 128 (a diffuse-only scene may go to 25)
    mi.Render(mi.Scene(S.cornell_box(32, 32, 2, max_depth=25))).run()


def test_crop_window(mi, oracle, golden_scenes):
    """A crop window of a larger frame (Film cropOffsetX/Y, cropWidth/Height; perspective.cpp:129-152): only the sample-to-camera matrix changes, so the HIP
    path stays bit-exact against the oracle; against the reference a couple of paths fork (the matrix is composed in float there)."""
    name = "cornell_crop"; sc = golden_scenes[name]; gs = mi.Scene(sc); orc = oracle.Oracle(sc); r = mi.Render(gs)
    r.run(); film = r.read_film(0); ofilm, _ = orc.render_image(threads=4)
    assert (bits(film) == bits(ofilm)).all()
    ref_film = np.load(os.path.join(GOLDEN, name + "_image.npz"))["film"]
    assert np.linalg.norm(film[..., :3] - ref_film[..., :3]) / np.linalg.norm(ref_film[..., :3]) < 5e-3
    gd = np.load(os.path.join(GOLDEN, name + "_samples.npz"))
    got = r.samples(gd["pairs"]); err = np.abs(got - gd["li"]).max(1) / (np.abs(gd["li"]).max(1) + 1e-6)
    assert (err < 2e-4).mean() > 0.998


def test_device_sincosf_equals_glibc(mi):
    """pt_device.h glibcSincosf (fp64 restatement of glibc's sincosf, the reference's math::sincos) against the host's glibc, bit for bit:
    every float of a dense sweep over the arguments the warps produce ([-pi/4, 3 pi/4] for the concentric disk, [0, 2 pi] for sphere / cone /
    cylinder sampling) plus random bit patterns in [-8, 8].  scripts/check_sincosf.c is the exhaustive version of this test for the CPU restatement."""
    import ctypes
    libm = ctypes.CDLL("libm.so.6"); libm.sincosf.argtypes = [ctypes.c_float, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]
    rng = np.random.default_rng(11)
    x = np.concatenate([np.linspace(-0.8, 6.4, 200001, dtype=np.float32), (rng.random(200000, dtype=np.float32) * 16 - 8).astype(np.float32),
                        np.float32([0.0, -0.0, 1e-5, 2.4e-4, 2.5e-4, np.pi / 4, np.nextafter(np.float32(np.pi / 4), np.float32(0)), np.pi / 2, np.pi, 2 * np.pi, 7.9999])])
    s, c = mi.device_sincosf(x)
    rs, rc = np.zeros_like(x), np.zeros_like(x); a, b = ctypes.c_float(), ctypes.c_float()
    for i in range(0, len(x), 7):       # every 7th value: ~57 k libm calls through ctypes
        libm.sincosf(float(x[i]), ctypes.byref(a), ctypes.byref(b)); rs[i], rc[i] = a.value, b.value
    sel = slice(0, len(x), 7)
    assert (bits(s[sel]) == bits(rs[sel])).all() and (bits(c[sel]) == bits(rc[sel])).all()


@pytest.mark.parametrize("name", ["expf", "logf", "powf", "tanf", "atanf", "atan2f", "acosf"])
def test_device_libm_equals_glibc(mi, name):
    """libm_glibc.h as compiled into the kernels against the host's glibc, bit for bit, on the argument ranges the path produces (scripts/check_libm.c is the exhaustive
    check of the same source compiled for the host): microfacet exponents and logs, roughness-derived powers, the tangent of Ward's azimuth ([0, 2 pi]) and of the
    rough-diffuse angles, arc functions of direction cosines."""
    import ctypes
    libm = ctypes.CDLL("libm.so.6"); f = getattr(libm, name); two = name in ("powf", "atan2f")
    f.restype = ctypes.c_float; f.argtypes = [ctypes.c_float] * (2 if two else 1)
    rng = np.random.default_rng(29); n = 60000
    lo, hi = {"expf": (-100, 80), "logf": (1e-30, 1e30), "powf": (0, 4), "tanf": (-64, 64), "atanf": (-1e6, 1e6), "atan2f": (-8, 8), "acosf": (-1, 1)}[name]
    x = (rng.random(n) * (hi - lo) + lo).astype(np.float32)
    if name in ("logf", "atanf"): x = (np.exp(rng.random(n) * 80 - 40) * (1 if name == "logf" else rng.choice([-1.0, 1.0], n))).astype(np.float32)
    x[:8] = np.float32([lo, hi, 1.0, 0.5, 1e-3, 0.0 if name != "logf" else 1.0, np.pi / 4 if name != "acosf" else 0.7, 2 * np.pi if name not in ("acosf",) else -0.7])
    y = None
    if two: y = ((rng.random(n) * 128 - 64) * rng.choice([1.0, 0.03125], n)).astype(np.float32) if name == "powf" else (rng.random(n) * 16 - 8).astype(np.float32)
    got = mi.device_libm(name, x, y)
    ref = np.float32([f(float(a), float(b)) for a, b in zip(x, y)]) if two else np.float32([f(float(a)) for a in x])
    same = (bits(got) == bits(ref)) | (np.isnan(got) & np.isnan(ref))
    assert same.all(), (name, x[~same][:4], got[~same][:4], ref[~same][:4])


@pytest.mark.parametrize("key", ["S1_cornell", "S2_veach", "S3_atrium", "S4_fog"])
def test_converged_images_vs_reference(mi, key):
    """SURVEY.md §8c item 11 / the north star's image tolerance: the three BASELINE scene classes at 240 x 135, Sobol, converged (1024 / 32768 / 32768 spp),
    rendered by the REFERENCE itself (fixtures tests/golden/converged/, generator tests/golden/make_golden.py --converged) -- once as shipped
    (-ffast-math) and once from the same sources under strict IEEE arithmetic.  The HIP film must be within 1e-4 relative L2 of the reference.
    The fixture also records how far the reference's two builds are from EACH OTHER (S1 3.6e-5, S2 6.9e-5, S3 6.7e-5): that is the floor any
    implementation that is not the same binary can reach against the fast-math build; against the strict build the HIP path is an order of magnitude closer.
    S4_fog: the volumetric loop (volpath over the fog_box room with the sensor inside a medium, 2048 spp)."""
    from tests.golden.make_golden import converged_scene
    fx = np.load(os.path.join(GOLDEN, "converged", key + ".npz")); sc = converged_scene(key)
    assert int(fx["spp"]) == sc.spp
    r = mi.Render(mi.Scene(sc)); r.run(); img = r.read_film(2).astype(np.float64)

    def rel(a, b):
        return float(np.sqrt(((a - b) ** 2).sum() / (b ** 2).sum()))
    e_fast, e_strict, floor = rel(img, fx["fast"].astype(np.float64)), rel(img, fx["strict"].astype(np.float64)), rel(fx["strict"].astype(np.float64), fx["fast"].astype(np.float64))
    print(f"{key}: HIP vs reference (fast-math build) {e_fast:.3g}, vs reference (strict build) {e_strict:.3g}; reference fast vs strict {floor:.3g}")
    assert e_strict <= 1e-4
    assert e_fast <= max(1e-4, 1.25 * floor)


@pytest.mark.parametrize("name", ["layered_room", "layered_room_strict_indep"])
def test_bsdf_adapters(mi, oracle, golden_scenes, name):
    """`bumpmap` (bitmap displacement under a `scale` texture: bilinear gradient of MIP level 0; grid displacement: finite differences),
    `normalmap`, `mixturebsdf` (2 and 3 children, weights rescaled to sum 1, twosided), bumpmap(mixture), mask(bumpmap): src/bsdfs/bumpmap.cpp, normalmap.cpp,
    mixturebsdf.cpp, src/textures/scale.cpp.  Against the oracle (plastic / diffuse lobes are libm-free; the rough conductors are tolerance-pinned), the reference's
    own samples -- both builds -- and its film."""
    sc = golden_scenes[name]; gs = mi.Scene(sc); orc = oracle.Oracle(sc); r = mi.Render(gs)
    gd = np.load(os.path.join(GOLDEN, name + "_samples.npz")); st_ = np.load(os.path.join(GOLDEN, "strict", name + ".npz"))
    rng = np.random.default_rng(23); n = 20000
    pairs = np.stack([rng.integers(0, sc.width, n), rng.integers(0, sc.height, n), rng.integers(0, sc.spp, n)], 1).astype(np.uint32)
    ref = orc.render_samples(pairs)["li"]; got = r.samples(pairs)
    err = np.abs(got - ref).max(1) / (np.abs(ref).max(1) + 1e-6)
    assert bit_share(got, ref, "bsdf_adapters " + name) >= 0.9999 and (err < 1e-4).mean() > 0.995 and np.median(err) < 1e-7, (err < 1e-4).mean()
    got = r.samples(gd["pairs"])
    err = np.abs(got - gd["li"]).max(1) / (np.abs(gd["li"]).max(1) + 1e-6)            # the reference as shipped (-ffast-math)
    assert (err < 1e-4).mean() > 0.99 and np.median(err) < 1e-6
    err = np.abs(got - st_["li"]).max(1) / (np.abs(st_["li"]).max(1) + 1e-6)          # the same sources, strict IEEE build
    assert (err < 1e-4).mean() > 0.998 and np.median(err) < 1e-7
    r.run(); film = r.read_film(0); ofilm, cnt = orc.render_image(threads=4); st = r.stats()
    assert np.linalg.norm(film[..., :3] - ofilm[..., :3]) / np.linalg.norm(ofilm[..., :3]) < 2e-4
    assert abs(st["rays"] - int(cnt[0])) / cnt[0] < 1e-3
    ref_film = np.load(os.path.join(GOLDEN, name + "_image.npz"))["film"]
    assert np.linalg.norm(film[..., :3] - ref_film[..., :3]) / np.linalg.norm(ref_film[..., :3]) < 2e-3      # 16 / 8 spp against the fast-math build: a few forked paths
    if name == "layered_room":       # validation of the nesting rules
        S = mi.scenes
        def broken(edit):
            bad = type(sc)(sc); bad["bsdfs"] = [dict(b) for b in sc.bsdfs]; edit(bad["bsdfs"]); return bad
        bump = [i for i, b in enumerate(sc.bsdfs) if b["type"] == S.BSDF_BUMPMAP]; mix = [i for i, b in enumerate(sc.bsdfs) if b["type"] == S.BSDF_MIXTURE]
        with pytest.raises(mi.MiError, match="bumpmap / normalmap nests"):
            mi.Scene(broken(lambda B: B[bump[0]].update(distr=bump[1])))
        with pytest.raises(mi.MiError, match="displacement texture"):
            mi.Scene(broken(lambda B: B[bump[0]].update(texture=-1)))
        with pytest.raises(mi.MiError, match="children of a mixturebsdf"):
            mi.Scene(broken(lambda B: B[mix[0]].update(reflectance=(float(bump[0]), B[mix[0]]["reflectance"][1], 0.0))))
        with pytest.raises(mi.MiError, match="texture coordinates are required"):
            bad = type(sc)(sc); bad["shapes"] = [dict(s) for s in sc.shapes]; bad["shapes"][0]["has_uv"] = 0; mi.Scene(bad)


@pytest.mark.parametrize("name", ["cornell_small", "atrium_small", "instanced_garden", "textured_shapes", "bunny_box"])
def test_scene_ray_intersect_full_records(mi, oracle, golden_scenes, name):
    """`bool Scene::rayIntersect(const Ray &, Intersection &)` for a batch of rays (mi_scene_ray_intersect; include/mitsuba/render/scene.h:187-243 over
    fillIntersectionRecord, skdtree.h:343-428): t, p, geometric and shading frame, uv, wi, primitive / instance / material / emitter of every hit equal the
    oracle's record bit for bit (packet scenes, BVH scenes, smooth normals, instances, analytic shapes with their own parameterisations)."""
    sc = golden_scenes[name]; gs = mi.Scene(sc); orc = oracle.Oracle(sc); rng = np.random.default_rng(31); n = 4000
    pos = rng.random((n, 2)).astype(np.float32) * np.array([sc.width, sc.height], np.float32)
    rays = gs.camera_rays(pos)                                     # camera rays ...
    recs = gs.ray_intersect(rays)
    sec = []                                                       # ... and rays leaving the first hits in random directions
    for i in range(0, n, 4):
        if recs["valid"][i]:
            d = rng.normal(size=3); d /= np.linalg.norm(d); sec.append(np.concatenate([recs["p"][i], [1e-4], d, [np.inf]]))
    rays = np.concatenate([rays, np.array(sec, np.float32)]); recs = gs.ray_intersect(rays)
    nhit = 0
    for i in range(len(rays)):
        ok, h = orc.intersect(rays[i])
        assert ok == bool(recs["valid"][i]), i
        if not ok: continue
        nhit += 1; r = recs[i]
        mine = np.concatenate([[r["t"]], r["p"], r["ng"], r["ns"], r["s"], r["bary"], r["wi"]]).astype(np.float32)
        ref = np.concatenate([h[0:1], h[1:4], h[4:7], h[7:10], h[10:13], h[13:15], h[15:18]]).astype(np.float32)
        assert (bits(mine) == bits(ref)).all(), (i, mine, ref)
        if int(r["prim"]) < len(sc.idx): assert (bits(r["uv"]) == bits(h[21:23])).all(), (i, r["uv"], h[21:23])
        else: assert np.allclose(r["uv"], h[21:23], atol=2e-6)            # analytic shapes: atan2 / acos of their parameterisations (device math library vs libm)
        assert int(r["instance"]) == int(h[20])
        si = int(h[19]); first = sc.shapes[si]["first_tri"] if si < len(sc.shapes) else len(sc.idx) + (si - len(sc.shapes))
        assert int(r["prim"]) == (first + int(h[18]) if si < len(sc.shapes) else first)
    assert nhit > len(rays) // 3


@pytest.mark.parametrize("name", ["veach_small", "atrium_small", "instanced_garden", "cbox_shapes", "bunny_box", "textured_shapes"])
def test_both_tree_node_kinds(mi, golden_scenes, name, monkeypatch):
    """The tree behind Scene::rayIntersect comes in two node kinds (binary nodes with float boxes; 4-wide nodes with 8-bit quantised child boxes, trace.h); the
    builder picks one by scene size (scene_build.cpp), MI355PT_BVH2 = 1 / 0 forces binary / wide.  Both walk supersets of the triangles the ray can hit and run
    the same exact triangle test: every radiance sample is the same bit for bit with either, and the big-scene fixtures (which the builder gives wide nodes
    by default) agree with the strict-IEEE build of the reference."""
    monkeypatch.setenv("MI355PT_NO_PACKET", "1")
    sc = golden_scenes[name]; gd = np.load(os.path.join(GOLDEN, name + "_samples.npz")); got = {}
    for kind, flag in (("binary", "1"), ("wide", "0")):
        monkeypatch.setenv("MI355PT_BVH2", flag)
        got[kind] = mi.Render(mi.Scene(sc)).samples(gd["pairs"])
    assert (bits(got["binary"]) == bits(got["wide"])).all()
    if name in ("atrium_small", "bunny_box"):        # atrium: the lat-long lookups use the device's atan2 / acos (test_envmap_atrium) -> not every sample bit-equal
        st = np.load(os.path.join(GOLDEN, "strict", name + ".npz"))
        err = np.abs(got["wide"] - st["li"]).max(1) / (np.abs(st["li"]).max(1) + 1e-6)
        assert bit_share(got["wide"], st["li"], "tree_node_kinds " + name) > 0.9999 and (err < 1e-4).mean() > 0.99


@pytest.mark.parametrize("name", ["fog_box", "fog_box_global", "fog_box_global_hide", "fog_mis", "fog_mis_global", "fog_mis_global_hide", "fog_constant", "fog_constant_simple_indep", "fog_pane", "fog_pane_mis", "fog_dusty", "fog_dusty_mis"])
def test_volpath_simple(mi, oracle, golden_scenes, name):
    """SimpleVolumetricPathTracer::Li (src/integrators/path/volpath_simple.cpp) over homogeneous media (src/medium/homogeneous.cpp: balance / single /
    manual distance sampling; isotropic and Henyey-Greenstein phase functions), `null` boundaries, a dielectric block with an interior medium, a `null` sphere, the
    sensor inside a medium; emitter sampling attenuated by Scene::evalTransmittance (scene.cpp:650-713) in k_shadow_vol.  exp / log go through the double-precision
    routines on every side (math.h:185-195), so the radiance samples equal the oracle's and those of the strict-IEEE build of the reference bit for bit.
    fog_mis*: the same rooms through VolumetricPathTracer::Li (src/integrators/path/volpath.cpp): multiple importance sampling between emitter sampling and
    phase-function / BSDF sampling, emitters found through index-matched boundaries (rayIntersectAndLookForEmitter; second record kind of k_shadow_volmis).
    fog_pane*: a thin glass pane (thindielectric) in the room: its ENull transmission lets emitter sampling and the emitter search look through it, attenuated
    (scene.cpp:679-685, volpath.cpp:399-402); volpath_simple samples it through the reference's pdf-less overload, which takes the SIGNED cosine (thindielectric.cpp:263).
    fog_dusty*: the pane as a mixturebsdf of the thin glass and a diffuse film: the walks see weight x the glass' pass-through value (mixturebsdf.cpp:176-183), and both
    MixtureBSDF::sample overloads call the child WITH a pdf, so the signed-cosine quirk does not apply to it.
    fog_constant*: under a `constant` environment emitter (no trigonometry: bit-exact as well; its density needs the cosine to the spawning vertex' normal)."""
    sc = golden_scenes[name]; gd = np.load(os.path.join(GOLDEN, name + "_samples.npz")); st = np.load(os.path.join(GOLDEN, "strict", name + ".npz"))
    gs = mi.Scene(sc); r = mi.Render(gs); orc = oracle.Oracle(sc)
    got = r.samples(gd["pairs"]); ref = orc.render_samples(gd["pairs"])["li"]
    same = (bits(got) == bits(ref)).all(1)
    assert same.mean() > 0.999 and np.allclose(got, ref, rtol=1e-5, atol=1e-7), same.mean()          # (a double-rounding difference of the device's exp / log is possible in principle)
    assert (bits(got) == bits(st["li"])).all(1).mean() > 0.999                                          # the reference itself, strict build
    err = np.abs(got - gd["li"]).max(1) / (np.abs(gd["li"]).max(1) + 1e-6)                             # the reference as shipped (-ffast-math)
    assert (err < 1e-4).mean() > 0.995 and np.median(err) < 1e-6
    rng = np.random.default_rng(5); n = 20000
    pairs = np.stack([rng.integers(0, sc.width, n), rng.integers(0, sc.height, n), rng.integers(0, sc.spp, n)], 1).astype(np.uint32)
    got = r.samples(pairs); ref = orc.render_samples(pairs)["li"]
    assert (bits(got) == bits(ref)).all(1).mean() > 0.999 and np.allclose(got, ref, rtol=1e-5, atol=1e-7)
    r.clear(); r.run(); film = r.read_film(0); ofilm, cnt = orc.render_image(threads=4); stt = r.stats()
    assert np.linalg.norm(film[..., :3] - ofilm[..., :3]) / np.linalg.norm(ofilm[..., :3]) < 1e-6
    assert stt["rays"] == int(cnt[0]) and stt["shadow_rays"] == int(cnt[1]) and stt["path_length_sum"] == int(cnt[2])
    ref_film = np.load(os.path.join(GOLDEN, name + "_image.npz"))["film"]                              # the reference's own image
    assert np.linalg.norm(film[..., :3] - ref_film[..., :3]) / np.linalg.norm(ref_film[..., :3]) < 1e-5
    ro = mi.Render(gs, opacity=True); ro.run(); oo = oracle.Oracle(sc, opacity=True).render_image(threads=4)[0]      # EOpacity: alpha of sensor rays that end in the fog, hit nothing, or hit a medium-transition shape (1 - transmittance of what lies behind, records.inl:124-137)
    assert np.allclose(ro.read_film(0)[..., 3], oo[..., 3], rtol=1e-6, atol=1e-6)
    assert (bits(ro.read_film(0)[..., :3]) == bits(film[..., :3])).all()                            # ... and the radiance does not notice


@pytest.mark.parametrize("name", ["fog_layered", "fog_layered_mis", "fog_layered_procedural", "fog_masked", "fog_masked_mis"])
def test_volumetric_bsdf_adapters(mi, oracle, golden_scenes, name):
    """mixturebsdf / bumpmap / normalmap (and bumpmap(mixture)) inside volpath_simple / volpath: the layered room filled with fog, a `null` sphere of haze over the
    mound (WRAP variants of k_shade_vol / k_shade_volmis).  Tolerances as test_bsdf_adapters (the rough conductors' libm calls); ray counters equal the oracle's.
    Adapters over a `null` / `thindielectric` are refused in volumetric renders (their ENull lobe would have to be evaluated inside the transmittance walks).
    fog_masked*: `mask` in the fogged open scene -- its ENull lobe attenuates the transmittance walks and the emitter search by 1 - opacity, the opacity texture looked
    up at the walk's uv ((0, 0) on a mesh without texture coordinates, skdtree.cpp:182-184); volpath_simple samples it through the pdf-less overload (mask.cpp:152-172)."""
    sc = golden_scenes[name]; gs = mi.Scene(sc); orc = oracle.Oracle(sc); r = mi.Render(gs)
    gd = np.load(os.path.join(GOLDEN, name + "_samples.npz")); st_ = np.load(os.path.join(GOLDEN, "strict", name + ".npz"))
    rng = np.random.default_rng(29); n = 20000
    pairs = np.stack([rng.integers(0, sc.width, n), rng.integers(0, sc.height, n), rng.integers(0, sc.spp, n)], 1).astype(np.uint32)
    ref = orc.render_samples(pairs)["li"]; got = r.samples(pairs)
    err = np.abs(got - ref).max(1) / (np.abs(ref).max(1) + 1e-6)
    assert (bits(got) == bits(ref)).all(1).mean() > 0.6 and (err < 1e-4).mean() > 0.995 and np.median(err) < 1e-7, ((bits(got) == bits(ref)).all(1).mean(), (err < 1e-4).mean())
    got = r.samples(gd["pairs"])
    err = np.abs(got - gd["li"]).max(1) / (np.abs(gd["li"]).max(1) + 1e-6)            # the reference as shipped (-ffast-math)
    assert (err < 1e-4).mean() > 0.99 and np.median(err) < 1e-6
    err = np.abs(got - st_["li"]).max(1) / (np.abs(st_["li"]).max(1) + 1e-6)          # the same sources, strict IEEE build
    assert (err < 1e-4).mean() > 0.998 and np.median(err) < 1e-7
    r.clear(); r.run(); film = r.read_film(0); ofilm, cnt = orc.render_image(threads=4); st = r.stats()
    assert np.linalg.norm(film[..., :3] - ofilm[..., :3]) / np.linalg.norm(ofilm[..., :3]) < 2e-4
    assert abs(st["rays"] - int(cnt[0])) / cnt[0] < 1e-3 and abs(st["shadow_rays"] - int(cnt[1])) / cnt[1] < 1e-3
    ref_film = np.load(os.path.join(GOLDEN, name + "_image.npz"))["film"]
    assert np.linalg.norm(film[..., :3] - ref_film[..., :3]) / np.linalg.norm(ref_film[..., :3]) < 2e-3
    if name == "fog_layered":
        S = mi.scenes
        bad = type(sc)(sc); bad["bsdfs"] = [dict(b) for b in sc.bsdfs]
        null = [i for i, b in enumerate(sc.bsdfs) if b["type"] == S.BSDF_NULL][0]; bump = [i for i, b in enumerate(sc.bsdfs) if b["type"] == S.BSDF_BUMPMAP][0]
        bad["bsdfs"][bump]["distr"] = null
        with pytest.raises(RuntimeError, match="null / thindielectric BSDF inside a bumpmap"):
            mi.Render(mi.Scene(bad))


@pytest.mark.parametrize("name", ["fog_sky", "fog_sky_simple", "fog_sky_global_hide"])
def test_volumetric_under_envmap(mi, oracle, golden_scenes, name):
    """volpath / volpath_simple under an environment map: the sky seen through media (EWA-filtered lookup for the sensor ray, volpath.cpp:181-192), emitter sampling of
    the map attenuated by the media, and -- volpath -- the map found by the emitter search behind index-matched boundaries (volpath.cpp:421-426).  The lat-long lookups
    use the device's atan2 / acos (as in test_envmap_atrium), so samples that touch the map are tolerance-pinned; the rest stays bit-exact."""
    sc = golden_scenes[name]; gd = np.load(os.path.join(GOLDEN, name + "_samples.npz")); st = np.load(os.path.join(GOLDEN, "strict", name + ".npz"))
    gs = mi.Scene(sc); r = mi.Render(gs); orc = oracle.Oracle(sc)
    got = r.samples(gd["pairs"]); ref = orc.render_samples(gd["pairs"])["li"]
    err = np.abs(got - ref).max(1) / (np.abs(ref).max(1) + 1e-6)
    assert (bits(got) == bits(ref)).all(1).mean() > 0.5 and (err < 1e-4).mean() > 0.99 and np.median(err) < 1e-6, ((bits(got) == bits(ref)).all(1).mean(), (err < 1e-4).mean())
    err = np.abs(got - st["li"]).max(1) / (np.abs(st["li"]).max(1) + 1e-6)                              # the reference itself, strict build
    assert (err < 1e-4).mean() > 0.99 and np.median(err) < 1e-6
    r.clear(); r.run(); film = r.read_film(0); ofilm, cnt = orc.render_image(threads=4); stt = r.stats()
    assert np.linalg.norm(film[..., :3] - ofilm[..., :3]) / np.linalg.norm(ofilm[..., :3]) < 2e-3
    assert abs(stt["rays"] - int(cnt[0])) / cnt[0] < 1e-3 and abs(stt["shadow_rays"] - int(cnt[1])) / cnt[1] < 1e-3
    ref_film = np.load(os.path.join(GOLDEN, name + "_image.npz"))["film"]                              # the reference's own image
    assert np.linalg.norm(film[..., :3] - ref_film[..., :3]) / np.linalg.norm(ref_film[..., :3]) < 2e-3


def test_volpath_simple_refusals(mi, golden_scenes):
    """what the volumetric stages are not built for is refused by name, never approximated"""
    S = mi.scenes
    sc = golden_scenes["open_constant"]
    with pytest.raises(RuntimeError, match="integrators path"):
        mi.Render(mi.Scene(golden_scenes["cornell_small"]), integrator=7)
    # a scene without media through the volumetric loop = the same estimator without MIS: converges to the same image (loose check on the mean).  The Cornell box
    # commits as a triangle packet; the volumetric stages walk its tree instead (decided per render, no environment switch needed)
    sc = S.cornell_box(64, 36, 64); gs = mi.Scene(sc)
    a = mi.Render(gs); a.run(); b = mi.Render(gs, integrator=S.INTEGRATOR_VOLPATH_SIMPLE); b.run(); c = mi.Render(gs, integrator=S.INTEGRATOR_VOLPATH); c.run()
    fa, fb, fc = a.read_film(0), b.read_film(0), c.read_film(0)
    assert abs(fa[..., :3].mean() - fb[..., :3].mean()) / fa[..., :3].mean() < 0.05
    # ... and volpath without media IS path: same sampler requests, same estimator (volpath.cpp vs path.cpp) -> the same film up to the operation order of the weights
    assert np.linalg.norm(fa[..., :3] - fc[..., :3]) / np.linalg.norm(fa[..., :3]) < 1e-5


@pytest.mark.parametrize("integrator", ["volpath_simple", "volpath"])
def test_volumetric_full_size_properties(mi, oracle, integrator):
    """The volumetric stages at a BASELINE film size (1080p, two 8-plane batches on two streams, 16 k segments, the 2 x cap shadow queue): spot samples equal the
    oracle's bit for bit; the film of [0, 16) equals the films of [0, 8) and [8, 16) accumulated one after the other bit for bit (sample-range additivity, the
    reference's per-pixel accumulation order); a second render reproduces the first; the weight channel counts the samples."""
    S = mi.scenes
    sc = S.fog_box(1920, 1080, 16, global_fog=True, integrator=S.INTEGRATOR_VOLPATH if integrator == "volpath" else S.INTEGRATOR_VOLPATH_SIMPLE)
    gs = mi.Scene(sc); r = mi.Render(gs, planes_per_batch=4); orc = oracle.Oracle(sc)
    rng = np.random.default_rng(77); n = 4000
    pairs = np.stack([rng.integers(0, sc.width, n), rng.integers(0, sc.height, n), rng.integers(0, sc.spp, n)], 1).astype(np.uint32)
    got = r.samples(pairs); ref = orc.render_samples(pairs)["li"]
    assert (bits(got) == bits(ref)).all(1).mean() > 0.999 and np.allclose(got, ref, rtol=1e-5, atol=1e-7)
    r.clear(); r.run(); full = r.read_film(0).copy(); st = r.stats()
    r.clear(); r.run(s0=0, s1=8); r.run(s0=8, s1=16); parts = r.read_film(0)
    assert (bits(full[1:-1, 1:-1, :3]) == bits(parts[1:-1, 1:-1, :3])).mean() > 0.9999
    r.clear(); r.run(); again = r.read_film(0)
    assert (bits(full[1:-1, 1:-1]) == bits(again[1:-1, 1:-1])).mean() > 0.9999
    assert np.isfinite(full).all() and abs(full[..., 4].sum() / (sc.width * sc.height * 16) - 1) < 1e-3 and st["samples"] == sc.width * sc.height * 16
    assert st["rays"] / st["samples"] > 4 and st["shadow_rays"] > 0


def test_scene_file_with_media(mi, oracle):
    """A hand-written scene FILE (tests/golden/scenes/fog_ball.xml) through the XML front end: `volpath`, three homogeneous media (hg / isotropic, sigmaT + albedo,
    `scale`, strategy `single`), a medium transition without a BSDF (gets `null`), a dielectric cube with a scattering interior, the sensor inside a medium, an area
    and a point light.  Radiance samples equal the oracle's bit for bit; films agree; ray counters equal."""
    X = __import__("importlib").import_module("mitsuba-im_amd.xml_scene")
    sc = X.load_scene(os.path.join(GOLDEN, "scenes", "fog_ball.xml"))
    assert sc.integrator == mi.scenes.INTEGRATOR_VOLPATH and len(sc.media) == 3 and sc.sensor_medium >= 0
    gs = mi.Scene(sc); r = mi.Render(gs); orc = oracle.Oracle(sc)
    rng = np.random.default_rng(9); n = 6000
    pairs = np.stack([rng.integers(0, sc.width, n), rng.integers(0, sc.height, n), rng.integers(0, sc.spp, n)], 1).astype(np.uint32)
    got = r.samples(pairs); ref = orc.render_samples(pairs)["li"]
    assert (bits(got) == bits(ref)).all(1).mean() > 0.999 and np.allclose(got, ref, rtol=1e-5, atol=1e-7)
    r.clear(); r.run(); film = r.read_film(0); ofilm, cnt = orc.render_image(threads=4); st = r.stats()
    assert np.linalg.norm(film[..., :3] - ofilm[..., :3]) / np.linalg.norm(ofilm[..., :3]) < 1e-6
    assert st["rays"] == int(cnt[0]) and st["shadow_rays"] == int(cnt[1]) and st["path_length_sum"] == int(cnt[2])


def test_batch_size_falls_back_when_memory_is_short(mi, monkeypatch):
    """mi_render_run sizes its path pools for 64 M paths in flight; when the card has no room for that (MI355PT_POOL_LIMIT stands in for a failing hipMalloc) it halves
    the automatic batch until the pools fit.  The film does not depend on how the sample planes are cut into batches: bit-identical to the unlimited render."""
    sc = mi.scenes.cornell_box(640, 360, 64); gs = mi.Scene(sc)
    a = mi.Render(gs); a.run(); fa = a.read_film(0)
    monkeypatch.setenv("MI355PT_POOL_LIMIT", str(300 << 20))                  # 300 MB per pool: ~1.4 M paths instead of the 7.4 M this job would take per batch
    b = mi.Render(gs); b.run(); fb = b.read_film(0)
    assert (bits(fa) == bits(fb)).all()
    monkeypatch.setenv("MI355PT_POOL_LIMIT", "1000")                          # nothing fits: the error of the last attempt comes back
    with pytest.raises(RuntimeError, match="MI355PT_POOL_LIMIT"):
        mi.Render(gs).run()
    # a handle that HAS pools and then fails to grow them: no queue pointer survives the failed re-allocation -- the next run allocates afresh, the film and the
    # ray counters are those of an undisturbed render (the retry used to leave freed buffers behind)
    monkeypatch.delenv("MI355PT_POOL_LIMIT")
    c = mi.Render(gs, planes_per_batch=1); c.run(s1=1); first = c.stats()["rays"]; assert first > 0
    monkeypatch.setenv("MI355PT_POOL_LIMIT", "1000")
    with pytest.raises(RuntimeError, match="MI355PT_POOL_LIMIT"):
        c.samples(np.asarray([[x % 640, (x // 640) % 360, 0] for x in range(640 * 360 * 2)], np.uint32))      # more paths than the pool holds -> re-allocation -> refused
    assert c.stats()["rays"] == first                                         # the counters of the released pools are kept
    monkeypatch.delenv("MI355PT_POOL_LIMIT")
    c.clear(); c.run(); fc = c.read_film(0)
    assert (bits(fa) == bits(fc)).all() and c.stats()["rays"] == a.stats()["rays"]
