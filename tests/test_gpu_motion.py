"""GPU (MI355X): the frame mark (mi_scene_mark_frame) and the prevPosition / motion field channels (include/mi355pt.h, csrc/kernels_field.hip) against the NumPy model
of their definition (tests/motion_model.py) on the census scene: per sample bit for bit, marks and edits composing, the field film, the temporal denoiser fed the
prevPosition channel, the refusals, and the read-back of the marked tables."""
import ctypes as C
import numpy as np
import pytest
from tests import adaptive_model as AM
from tests import film_model as FM
from tests import motion_model as mm
from tests import temporal_model as tm

pytestmark = pytest.mark.gpu
f32 = np.float32
UNDEF = (-1.0, 2.5, 7.0)
KINDS = ["position", "prevPosition", "motion"]


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def device_records(oracle, gs, pairs):
    """the pinned pieces, as test_gpu_fields.records_of: oracle film positions -> device camera rays -> device intersection records, in the model's layout"""
    pos = oracle.Oracle(gs.sc).render_samples(pairs)["pos"]; r = gs.ray_intersect(gs.camera_rays(pos))
    return dict(hit=r["valid"] != 0, inst=r["instance"].astype(np.int64), prim=r["prim"].astype(np.int64), u=r["bary"][:, 0].copy(), v=r["bary"][:, 1].copy(), p=r["p"].copy()), pos


def now(gs):
    """the state a mark would snapshot, with the library's own projection"""
    return mm.state(gs.sc, gs.world_to_pixel())


def edit(S, gs, sc0, step):
    pos, insts, cam = mm.census_edit(S, sc0, step)
    gs.update_geometry(pos, instances=insts); gs.update_camera(gs.sc.sample_to_camera, cam, gs.sc.near, gs.sc.far)


def check_fields(got, exp, cl=None, tag=""):
    for i, name in enumerate(KINDS):
        same = (bits(got[:, i]) == bits(exp[name])).all(1)
        if cl is not None:
            for k, sel in cl.items(): assert same[sel].all(), (tag, name, k, int((~same[sel]).sum()), got[sel, i][~same[sel]][:2], exp[name][sel][~same[sel]][:2])
        assert same.all(), (tag, name, int((~same).sum()), got[~same, i][:3], exp[name][~same][:3])


# ---------------------------------------------------------------------------------------------- 1: per sample against the model
def test_field_samples_equal_the_model(mi, oracle):
    """mark -> update_geometry(pos, instances) -> update_camera: position, prevPosition and motion of one sample per pixel equal the model bit for bit in every class
    of the census (each holds at least 8 samples on the device's own records); a miss is `undefined`.  The mark moved neither revision nor tree_builds."""
    S = mi.scenes; sc0 = mm.census_scene(S); gs = mi.Scene(mm.census_scene(S)); r = mi.Render(gs, fields=[(k, UNDEF) for k in KINDS]); pairs = mm.pixel_samples(sc0)
    rev = gs.revision(); gs.mark_frame(); assert gs.revision() == rev
    prev = now(gs); edit(S, gs, sc0, 1.0); cur = now(gs)
    rec, _ = device_records(oracle, gs, pairs); cl = mm.classify(gs.sc, prev, cur, rec); counts = {k: int(v.sum()) for k, v in cl.items()}
    print(f"[motion] census on the device's records {counts}"); assert all(c >= 8 for c in counts.values()), counts
    got = r.field_samples(pairs); assert got.shape == (len(pairs), 3, 3)
    check_fields(got, mm.fields(gs.sc.idx, prev, cur, rec, UNDEF), cl, "edit")
    for k in ("unmoved_mesh", "static_instance", "analytic"): assert (bits(got[cl[k], 1]) == bits(got[cl[k], 0])).all(), k
    for k in ("moved_mesh", "moved_instance", "deformed_member"): assert (np.abs(got[cl[k], 1] - got[cl[k], 0]).max(1) > 1e-3).all(), k


# ---------------------------------------------------------------------------------------------- 2: marks and edits compose
def test_marks_and_edits_compose(mi, oracle):
    """Never marked: prevPosition == position bit for bit and motion == 0, also after an edit.  One mark, two edits: previous is still the marked state.  A second mark:
    previous = current again; an edit after it is measured from the second mark (whose vertices the device copied from its own array)."""
    S = mi.scenes; sc0 = mm.census_scene(S); gs = mi.Scene(mm.census_scene(S)); r = mi.Render(gs, fields=[(k, UNDEF) for k in KINDS]); pairs = mm.pixel_samples(sc0)

    def still(tag):
        got = r.field_samples(pairs); hit = ~(bits(got[:, 0]) == bits(f32(UNDEF))).all(1); assert hit.sum() > 200
        assert (bits(got[hit, 1]) == bits(got[hit, 0])).all() and (bits(got[hit, 2]) == 0).all(), tag
    still("never marked"); edit(S, gs, sc0, 0.5); still("never marked, edited")
    gs.mark_frame(); prev = now(gs); still("marked, no edit")
    edit(S, gs, sc0, 1.0); edit(S, gs, sc0, 0.25); cur = now(gs); rec, _ = device_records(oracle, gs, pairs)
    check_fields(r.field_samples(pairs), mm.fields(gs.sc.idx, prev, cur, rec, UNDEF), None, "one mark, two edits")
    gs.mark_frame(); prev2 = now(gs); still("second mark")
    edit(S, gs, sc0, 1.0); cur2 = now(gs); rec2, _ = device_records(oracle, gs, pairs)
    got = r.field_samples(pairs); check_fields(got, mm.fields(gs.sc.idx, prev2, cur2, rec2, UNDEF), None, "after the second mark")
    assert not (bits(got[:, 1]) == bits(mm.fields(gs.sc.idx, prev, cur2, rec2, UNDEF)["prevPosition"])).all()      # not the first mark's


# ---------------------------------------------------------------------------------------------- 3: the field film
@pytest.mark.parametrize("spp,filt", [(1, 0), (4, 1)])
def test_prev_position_film(mi, oracle, spp, filt):
    """The raw prevPosition film of the edited scene equals film_model.put64 fed the model's per-sample values, within test_field_film's bound ((n + 2) 2^-24 sum |w v|
    per pixel and plane); layout 2 is the reference's develop of it exactly."""
    import tests.test_gpu_fields as TF
    S = mi.scenes; sc0 = mm.census_scene(S, spp=spp, filter_kind=filt); gs = mi.Scene(mm.census_scene(S, spp=spp, filter_kind=filt))
    gs.mark_frame(); prev = now(gs); edit(S, gs, sc0, 1.0); cur = now(gs)
    pairs = np.concatenate([mm.pixel_samples(sc0, k) for k in range(spp)]); rec, pos = device_records(oracle, gs, pairs)
    vals = mm.fields(gs.sc.idx, prev, cur, rec, UNDEF)["prevPosition"].astype(np.float64)
    orc = oracle.Oracle(gs.sc); ev, rad, b = AM.filter_table(oracle, orc)
    exp, mag, cnt = FM.put64(ev, rad, b, sc0.width, sc0.height, pos, vals)
    r = mi.Render(gs, planes_per_batch=2, fields=[("prevPosition", UNDEF)]); r.run()
    raw = r.read_fields(0); assert raw.shape == exp.shape
    TF.check_film(raw, exp, mag, cnt, f"prevPosition {spp} spp filter {filt}")
    inner = raw[b:raw.shape[0] - b, b:raw.shape[1] - b] if b else raw
    assert (bits(r.read_fields(2)) == bits(FM.develop32(inner))).all()


# ---------------------------------------------------------------------------------------------- 4: the temporal denoiser
def test_temporal_denoising_follows_a_spinning_instance(mi, oracle):
    """Three frames, 192 x 144, four new sample indices each; the crate at +x turns by 30 degrees per frame about its own axis and sinks by 0.2, so that its lid neither
    stays where it was nor slides in its own plane: every lid point further than 0.43 from the axis moves more than twice the temporal tolerance 0.15, and the surface a pixel sees lies more than
    three tolerances from the one it saw a frame earlier.  With a prevPosition field Render.denoise_temporal equals temporal_model.temporal_frame given the developed
    prevPosition channel as prev_position, and denoise_image_temporal on the read-back arrays, bit for bit -- output, history, widths.  On the pixels whose samples all
    stay on that lid the history count reaches 3 (exactly 3 where every counted tap held 2); the same frames on a render without the field leave 1 there (Pprev = P:
    the behaviour before the field existed)."""
    S = mi.scenes; w, h = 192, 144; sc0 = mm.census_scene(S, w, h, spp=12); gs = mi.Scene(mm.census_scene(S, w, h, spp=12))
    r = mi.Render(gs, spp=12, fields=[("shNormal", 0.0), ("position", 0.0), ("prevPosition", 0.0)]); r0 = mi.Render(gs, spp=12, fields=[("shNormal", 0.0), ("position", 0.0)])
    Hr, Hi, H0 = mi.History(w, h), mi.History(w, h), mi.History(w, h); hist = None; tp = 0.15
    kw = dict(iterations=2, sigma_color=4.0, sigma_normal=0.3, sigma_position=-0.05, max_history=32.0, temporal_sigma_position=tp, min_normal_dot=0.8)
    base = np.asarray(sc0.instances[1]["to_world"], np.float64); stay = np.ones((h, w), bool); lid = sc0.shapes[2]["first_tri"]; last = None
    for f in range(3):
        gs.mark_frame()
        gs.update_instances([sc0.instances[0], S.make_instance(0, S.translate(0.0, -0.2 * (f + 1), 0.0) @ base @ S.rotate((0, 1, 0), 30.0 * (f + 1)))])
        for rr in (r, r0): rr.clear(); rr.run(s0=4 * f, s1=4 * f + 4)
        film = r.read_film(2); fl = r.read_fields(2); N, P, Q = fl[..., 0:3], fl[..., 3:6], fl[..., 6:9]; M = gs.world_to_pixel()
        got = r.denoise_temporal(Hr, **kw); gres, gtp = r.last_denoise_sigma_position, r.last_temporal_sigma_position
        img, ires, itp = mi.denoise_image_temporal(Hi, film, N, P, None, Q, M, **kw)
        exp, eres, etp, hist = tm.temporal_frame(hist, film, N, P, None, Q, M, **kw)
        assert (bits(got) == bits(img)).all() and (bits(img) == bits(exp)).all(), f
        assert bits(f32(gres)) == bits(f32(ires)) == bits(f32(eres)) and bits(f32(gtp)) == bits(f32(itp)) == bits(f32(etp)) == bits(f32(tp))
        for H in (Hr, Hi):
            col, cnt = H.read(); assert (bits(col) == bits(hist["a"])).all() and (bits(cnt) == bits(hist["n"])).all(), f
        r0.denoise_temporal(H0, **kw)
        pairs = np.concatenate([mm.pixel_samples(sc0, k) for k in range(4 * f, 4 * f + 4)]); rec, _ = device_records(oracle, gs, pairs)
        on = (rec["hit"] & (rec["inst"] == 1) & (rec["prim"] >= lid) & (rec["prim"] < lid + 2)).reshape(4, h, w).all(0)
        stay &= on & (np.sqrt(((P.astype(np.float64) - Q) ** 2).sum(-1)) > 2 * tp)
        if last is not None: stay &= np.sqrt(((P.astype(np.float64) - last) ** 2).sum(-1)) > 3 * tp
        last = P.astype(np.float64)
    n_with = Hr.read()[1][stay]; n_without = H0.read()[1][stay]
    print(f"[motion] temporal: {int(stay.sum())} pixels stay on the turning lid; counts with the field min {n_with.min()} mean {n_with.mean():.3f} max {n_with.max()}, "
          f"share at 3: {(n_with == 3.0).mean():.3f}; without {n_without.min()} .. {n_without.max()}")
    assert stay.sum() >= 50
    assert n_with.max() == 3.0 and (n_with == 3.0).mean() > 0.5 and (n_with >= 2.0).mean() > 0.9
    assert (n_without == 1.0).all()


# ---------------------------------------------------------------------------------------------- 5: refusals
def test_refusals_by_name(mi):
    """A mark on an uncommitted scene; the new fields on an adaptive render (either order) and on a `devices` render of the host mirror."""
    L = mi.lib(); hdl = C.c_void_p(); L.check(L.L.mi_scene_create(C.byref(hdl)))
    with pytest.raises(mi.MiError, match="mi_scene_mark_frame: scene not committed") as e: L.check(L.L.mi_scene_mark_frame(hdl))
    assert e.value.code == 1; L.L.mi_scene_destroy(hdl)
    with pytest.raises(mi.MiError, match="mi_scene_mark_frame: null scene"): L.check(L.L.mi_scene_mark_frame(None))
    S = mi.scenes; gs = mi.Scene(mm.census_scene(S, spp=8))
    r = mi.Render(gs, fields=["position", "prevPosition"])
    with pytest.raises(mi.MiError, match="prevPosition") as e: r.set_adaptive()
    assert e.value.code == 3
    r = mi.Render(gs); r.set_adaptive()
    with pytest.raises(mi.MiError, match="motion") as e: r.set_fields(["motion"])
    assert e.value.code == 3
    r.set_fields(["distance"])      # what the refusal left: the other kinds still go through this call
    sc = mm.census_scene(S, spp=8); sc.fields = ["position", "motion"]
    with pytest.raises(mi.MiError, match="`motion`") as e: mi.api.HostIntegrator(mi.Scene(sc), devices=(0, 0))
    assert e.value.code == 3
    with pytest.raises(ValueError, match="unknown field"): mi.Render(gs, fields=["previousPosition"])


# ---------------------------------------------------------------------------------------------- 6: the marked tables
def test_read_geometry_of_the_previous_tables(mi):
    """Never marked: both tables are empty.  After mark and edit they equal what the current tables held before the edit -- the vertices as the shading records carry
    them (words 0..2, 4..6, 8..10 through the indices in words 19, 23, 27), rows 0..2 of every instance's to_world (words 0..11) -- and a replica carries them."""
    S = mi.scenes; sc0 = mm.census_scene(S); gs = mi.Scene(mm.census_scene(S))
    assert gs.read_geometry("prev_vertices").shape[0] == 0 and gs.read_geometry("prev_instances").shape[0] == 0
    shade0 = gs.read_geometry("tri_shade"); inst0 = gs.read_geometry("instances")
    gs.mark_frame(); edit(S, gs, sc0, 1.0)
    pv = gs.read_geometry("prev_vertices"); pi = gs.read_geometry("prev_instances"); shade1 = gs.read_geometry("tri_shade"); inst1 = gs.read_geometry("instances")
    assert pv.shape == (len(sc0.pos), 3) and pi.shape == (2, 12)
    assert (pi == inst0[:, :12]).all() and not (pi == inst1[:, :12]).all()
    for c, (w0, wi) in enumerate(((0, 19), (4, 23), (8, 27))):
        assert (pv[shade0[:, wi]] == shade0[:, w0:w0 + 3]).all(), c
    assert not all((pv[shade1[:, wi]] == shade1[:, w0:w0 + 3]).all() for w0, wi in ((0, 19), (4, 23), (8, 27)))
    assert (pv == bits(sc0.pos)).all()
    twin = gs.clone(0)
    assert (twin.read_geometry("prev_vertices") == pv).all() and (twin.read_geometry("prev_instances") == pi).all()
    twin.close()
