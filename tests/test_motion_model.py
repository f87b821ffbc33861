"""The model of the prevPosition / motion fields (tests/motion_model.py) on the census scene, without a GPU: the intersection records are the oracle's."""
import numpy as np
import pytest
from tests import motion_model as mm

f32 = np.float32
EPS = 2.0 ** -24


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


@pytest.fixture(scope="module")
def case(mi, oracle):
    """the census scene before and after its edit, the two states, and the oracle's records of one sample per pixel of the EDITED scene"""
    S = mi.scenes; sc = mm.census_scene(S); sc2 = mm.edited(S, sc); prev = mm.state(sc); cur = mm.state(sc2)
    rec, rays, _ = mm.oracle_records(oracle.Oracle(sc2), mm.pixel_samples(sc2))
    rec0, _, _ = mm.oracle_records(oracle.Oracle(sc), mm.pixel_samples(sc))
    return dict(S=S, sc=sc, sc2=sc2, prev=prev, cur=cur, rec=rec, rays=rays, rec0=rec0)


def test_census(case):
    """32 x 24 pixels, one sample each: at least 8 samples in every class -- moved mesh, unmoved part of the moved mesh, moved instance, deformed member, static
    instance, analytic, miss -- for the oracle's intersections."""
    sc2 = case["sc2"]; assert (sc2.width, sc2.height) == (32, 24) and len(case["rec"]["hit"]) == 32 * 24
    cl = mm.classify(sc2, case["prev"], case["cur"], case["rec"]); counts = {k: int(v.sum()) for k, v in cl.items()}
    print(f"[motion] census {counts}")
    assert set(counts) == set(mm.CLASSES) and all(c >= 8 for c in counts.values()), counts
    assert sum(counts.values()) == 32 * 24 - int((case["rec"]["hit"] & ~np.any([cl[k] for k in mm.CLASSES], 0)).sum())      # the rest: the light, static meshes
    vm = (bits(case["prev"]["pos"]) != bits(case["cur"]["pos"])).any(1); s0 = sc2.shapes[0]; sheet = vm[s0["first_vert"]:s0["first_vert"] + s0["vert_count"]]
    assert 0.4 < sheet.mean() < 0.6      # half the sheet's vertices move


def test_no_edit(case):
    """A mark with no edit: previous = current.  prevPosition == position bit for bit and motion == 0 on every hit (also how a never-marked scene behaves)."""
    sc = case["sc"]; st = case["prev"]; rec = case["rec0"]; hit = rec["hit"]; assert hit.sum() > 200
    f = mm.fields(sc.idx, st, st, rec, undefined=(-1.0, 2.5, 7.0))
    assert (bits(f["prevPosition"][hit]) == bits(rec["p"][hit])).all() and (bits(f["position"][hit]) == bits(rec["p"][hit])).all()
    assert (bits(f["motion"][hit]) == 0).all()
    for name in ("position", "prevPosition", "motion"): assert (bits(f[name][~hit]) == bits(f32([-1.0, 2.5, 7.0]))).all()


def test_what_did_not_move_keeps_its_bits(case):
    """After the edit: the unmoved part of the moved mesh, the static placement and the sphere have prevPosition == position bit for bit; their motion is the
    camera's alone (not zero: the camera moved)."""
    cl = mm.classify(case["sc2"], case["prev"], case["cur"], case["rec"]); f = mm.fields(case["sc2"].idx, case["prev"], case["cur"], case["rec"])
    for k in ("unmoved_mesh", "static_instance", "analytic"):
        assert (bits(f["prevPosition"][cl[k]]) == bits(f["position"][cl[k]])).all(), k
        assert (np.abs(f["motion"][cl[k]]).max(1) > 0).all(), k
    for k in ("moved_mesh", "moved_instance", "deformed_member"):
        assert (np.abs(f["prevPosition"][cl[k]] - f["position"][cl[k]]).max(1) > 1e-3).all(), k


def test_rigid_move_of_an_instance(case):
    """prevPosition of the moved placement's undeformed triangles equals Tprev Tcur^-1 P evaluated in float64 within k 2^-24 m, m = the largest coordinate magnitude
    entering the computation (ray origin, object-space corners, P, the translations of the two transforms).

    k from the operation count, every rounding taken as 2^-24 of at most 2 m (a partial sum of two coordinates).  Given (u, v, P) the formula is P + (Tprev b - Tcur b)
    with ONE b = bary(corners) for both sides (the corners did not move): two transforms of 3 multiplications + 3 additions, one subtraction, one addition = 14 roundings
    -> 28.  The exact value differs from the formula in exact arithmetic by (Rprev - Rcur)(b - Tcur^-1 P): the hit point the ray gave against the barycentric point, at
    most 2 sqrt(3) times their distance per component (two rotations).  Roundings between the ray and those two points: to_object on the origin 6 and on the direction 5,
    the hit point o + d t 2, to_world on it 6 (pulled back through a rotation), the Wald test's in-plane coordinates 4 and barycentrics 6, bary 7 (its b.x included) = 36;
    and the distance t enters both points: numerator 5, the plane constant 6, denominator 4, division 1 = 16, twice, divided by the cosine of incidence, which the test
    asserts to be at least 0.25 on these samples: 32 x 4 = 128.  (36 + 128) x 2 x 2 sqrt(3) = 1137; k = 28 + 1137 -> 1200."""
    k = 1200.0
    sc2 = case["sc2"]; rec = case["rec"]; cl = mm.classify(sc2, case["prev"], case["cur"], rec)["moved_instance"]; assert cl.sum() >= 8
    inst = rec["inst"][cl]; assert (inst == 1).all()
    cos = np.abs((case["rays"][cl, 4:7] * rec["ng"][cl]).sum(1)); assert cos.min() >= 0.25, cos.min()
    f = mm.fields(sc2.idx, case["prev"], case["cur"], rec)
    full = lambda m: np.vstack([np.asarray(m, np.float64), [0.0, 0.0, 0.0, 1.0]])
    Tp = full(case["prev"]["to_world"][1]); Tc = full(case["cur"]["to_world"][1]); P = rec["p"][cl].astype(np.float64)
    exp = (np.c_[P, np.ones(len(P))] @ (Tp @ np.linalg.inv(Tc)).T)[:, :3]
    corners = np.abs(case["cur"]["pos"][np.asarray(sc2.idx, np.int64)[rec["prim"][cl]]]).max()
    m = max(np.abs(case["rays"][cl, :3]).max(), corners, np.abs(P).max(), np.abs(Tp[:3, 3]).max(), np.abs(Tc[:3, 3]).max())
    err = np.abs(f["prevPosition"][cl].astype(np.float64) - exp).max()
    print(f"[motion] rigid move: max err {err:.3e}, bound {k * EPS * m:.3e} (m = {m:.3f}), displacement up to {np.abs(exp - P).max():.3f}")
    assert err <= k * EPS * m and np.abs(exp - P).max() > 0.1


def test_motion_is_the_reprojection_difference(case):
    """motion against a float64 evaluation of its definition from the model's own prevPosition: film positions within 1e-3 pixel, distances within 1e-5"""
    sc2 = case["sc2"]; rec = case["rec"]; hit = rec["hit"]; prev, cur = case["prev"], case["cur"]; f = mm.fields(sc2.idx, prev, cur, rec)
    def proj(M, q):
        M = np.asarray(M, np.float64).reshape(3, 4); h = np.c_[q.astype(np.float64), np.ones(len(q))] @ M.T; return h[:, :2] / h[:, 2:3]
    Q = f["prevPosition"][hit]; P = f["position"][hit]
    exp_xy = proj(prev["w2p"], Q) - proj(cur["w2p"], P)
    exp_d = np.linalg.norm(Q.astype(np.float64) - prev["origin"], axis=1) - np.linalg.norm(P.astype(np.float64) - cur["origin"], axis=1)
    assert np.abs(f["motion"][hit][:, :2] - exp_xy).max() < 1e-3 and np.abs(f["motion"][hit][:, 2] - exp_d).max() < 1e-5
    # a point behind the marked camera has no motion: `undefined`
    behind = dict(prev, w2p=-np.asarray(prev["w2p"], f32))
    g = mm.fields(sc2.idx, behind, cur, rec, undefined=(9.0, 9.0, 9.0))
    assert (g["motion"][hit] == 9.0).all() and (bits(g["prevPosition"][hit]) == bits(Q)).all()
