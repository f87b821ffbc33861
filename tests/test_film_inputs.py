"""CPU: the inputs of tests/test_gpu_film_units.py meet the conditions the film-unit tests rest on.  Every condition is on the INPUTS, computed with the oracle's filter
table for each of the six filters -- none on the code under test: the edge classes occur often enough, no cell of the isolated and single-thread layouts is touched by
two threads (which is what makes equal bits a fair demand), the footprints are the ones the spacing of 7 was chosen for, and an adaptive run over the isolated layout ends
in all three ways."""
import numpy as np
import pytest
from tests import adaptive_model as AM
from tests import film_inputs as FI
from tests import film_model as FM

f32 = np.float32
_cache = {}


def case(mi, oracle, kind):
    """(oracle handle, ev, radius, border) of filter `kind` on the 22 x 15 film"""
    if kind not in _cache:
        orc = oracle.Oracle(FI.scene(mi.scenes, kind)); _cache[kind] = (orc,) + AM.filter_table(oracle, orc)
    return _cache[kind]


def census(ev, rad, b, pos, val, owner_xy=None):
    """counts of the edge classes over the samples (pos [n, 2], val [n, 4]); owner_xy [n, 2]: the pixel whose thread puts the sample (box spill classes)"""
    c = dict(zero_weight=0, negative_weight=0, px_plus_one=0, clip_left=0, clip_right=0, clip_top=0, clip_bottom=0, empty=0, box_spill=0, box_no_spill_15=0)
    Wb, Hb = FI.W + 2 * b, FI.H + 2 * b
    ok = FM.accepted(val)
    for i in np.flatnonzero(ok):
        x0, x1, y0, y1, wx, wy = FM.footprint(ev, rad, b, FI.W, FI.H, pos[i, 0], pos[i, 1])
        posx, posy = FM.film_coord(pos[i, 0], b), FM.film_coord(pos[i, 1], b)
        if x0 > x1 or y0 > y1: c["empty"] += 1; continue
        c["zero_weight"] += int((wx == 0).any() or (wy == 0).any()); c["negative_weight"] += int((wx < 0).any() or (wy < 0).any())
        c["clip_left"] += int(np.ceil(f32(posx - rad)) < 0); c["clip_right"] += int(np.floor(f32(posx + rad)) > Wb - 1)
        c["clip_top"] += int(np.ceil(f32(posy - rad)) < 0); c["clip_bottom"] += int(np.floor(f32(posy + rad)) > Hb - 1)
        if owner_xy is not None:
            ox, oy = owner_xy[i]; fx, fy = pos[i, 0] - f32(ox), pos[i, 1] - f32(oy)
            c["px_plus_one"] += int(fx == 1 or fy == 1)
            inside = 0 <= fx <= 1 and 0 <= fy <= 1
            c["box_spill"] += int(inside and (x0 < ox + b or x1 > ox + b or y0 < oy + b or y1 > oy + b))
            c["box_no_spill_15"] += int((fx == f32(1.5e-5) and x0 == ox + b) or (fy == f32(1.5e-5) and y0 == oy + b))
    return c


def owners(n_planes):
    yy, xx = np.divmod(np.arange(FI.N_PIX), FI.W)
    return np.tile(np.stack([xx, yy], 1), (n_planes, 1))


@pytest.mark.parametrize("kind", range(6))
def test_census(mi, oracle, kind):
    orc, ev, rad, b = case(mi, oracle, kind); name = FI.FILTER_NAMES[kind]
    hb = int(np.floor(rad + f32(0.5))); assert hb <= 3 and b <= 3
    ipos, ival, iact = FI.isolated(); spos, sval, sact = FI.single(); dpos, dval = FI.dense()
    assert ipos.shape == (16, 330, 2) and spos.shape == (48, 330, 2) and dpos.shape == (8, 330, 2)
    assert iact.sum() == 12 and sact.sum() == 1 and FI.N_PIX == 330 and FI.N_PIX > 256 and FI.N_PIX % 256          # two workgroups, a ragged tail
    # values: the accepted ones in [2^-10, 2^10] with alpha out of {0, 0.5, 1}; every inactive pixel's samples are rejected, two planes of every active pixel too
    for val in (ival, sval, dval):
        ok = FM.accepted(val); v = val[ok]
        assert (v[:, :3] >= 2.0 ** -10).all() and (v[:, :3] <= 2.0 ** 10).all() and np.isin(v[:, 3], [0, 0.5, 1]).all()
    assert not FM.accepted(ival[:, ~iact]).any() and not FM.accepted(sval[:, ~sact]).any() and FM.accepted(sval[:, sact]).all()
    assert ((~FM.accepted(ival[:, iact])).sum(0) == 2).all()
    # the isolated layout's active samples lie inside or on the edge of the own pixel; the single layout's reach 2^20
    own = owners(16).reshape(16, 330, 2)[:, iact]; fr = ipos[:, iact] - own.astype(f32); assert (fr >= 0).all() and (fr <= 1).all()
    assert np.abs(spos).max() == 2.0 ** 20 and np.isfinite(spos).all() and np.isfinite(dpos).all()
    counts = {}
    for tag, pos, val, act in (("isolated", ipos, ival, iact), ("single", spos, sval, sact), ("dense", dpos, dval, None)):
        K = len(pos); o = owners(K)
        counts[tag] = census(ev, rad, b, pos.reshape(-1, 2), val.reshape(-1, 4), o)
        causes = FI.reject_cause(val); counts[tag]["causes"] = [int((causes == i).sum()) for i in range(5)]
        print(f"[film inputs] {name} {tag}: {counts[tag]}")
    iso, sgl, dns = counts["isolated"], counts["single"], counts["dense"]
    assert min(iso["causes"]) >= 8 and min(sgl["causes"]) >= 8 and min(dns["causes"]) >= 8
    assert iso["px_plus_one"] >= 8 and dns["px_plus_one"] >= 8
    # a boundary cell of weight exactly 0: where pos +- radius is an integer the last cell of the footprint reads table entry MI_FILTER_RES.  The radius is an integer for
    # every filter but the box (0.5 + 1e-5), whose boundary cells lie inside the radius
    if kind != 0: assert iso["zero_weight"] >= 8 and dns["zero_weight"] >= 8
    if kind >= 3: assert iso["negative_weight"] >= 8 and dns["negative_weight"] >= 8 and sgl["negative_weight"] >= 8
    if kind == 0: assert iso["box_spill"] >= 8 and iso["box_no_spill_15"] >= 8 and dns["box_spill"] >= 8 and dns["box_no_spill_15"] >= 8
    # a footprint cut by the film's edge and not empty: only samples OFF the film leave the border (b = ceil(radius - 0.5) cells), the box filter's only at exactly one
    # cell outside; the single-thread layout holds such samples at every edge and corner, the dense layout the bulk
    for k in ("clip_left", "clip_right", "clip_top", "clip_bottom"): assert sgl[k] >= 2 and sgl[k] + dns[k] >= 8, (k, sgl[k], dns[k])
    assert sgl["empty"] >= 8 and iso["empty"] == 0
    # the single-thread layout against k_adapt_accumulate's clamp to own +- hb: footprints that reach into the own block, and footprints that reach beyond it
    ox, oy = FI.SINGLE_PIXEL[0] + b, FI.SINGLE_PIXEL[1] + b; into = beyond = 0
    for p in spos[:, sact].reshape(-1, 2):
        x0, x1, y0, y1, _, _ = FM.footprint(ev, rad, b, FI.W, FI.H, p[0], p[1])
        if x0 > x1 or y0 > y1: continue
        into += int(x0 <= ox + hb and x1 >= ox - hb and y0 <= oy + hb and y1 >= oy - hb); beyond += int(x0 < ox - hb or x1 > ox + hb or y0 < oy - hb or y1 > oy + hb)
    assert into >= 4 and beyond >= 8, (into, beyond)


@pytest.mark.parametrize("kind", range(6))
def test_one_thread_per_cell(mi, oracle, kind):
    """isolated and single-thread layouts: no film cell is touched by two different threads, from the model's per-thread footprints; the isolated footprints are the ones
    the spacing was chosen for; developed weights of 0 and (filters with negative lobes) below 0 occur in the isolated film"""
    orc, ev, rad, b = case(mi, oracle, kind)
    for pos, val, act in (FI.isolated()[:3], FI.single()[:3]):
        K = len(pos); owner = np.tile(np.arange(FI.N_PIX), K)
        cells = FM.thread_cells(ev, rad, b, FI.W, FI.H, pos.reshape(-1, 2), val.reshape(-1, 4), owner)
        assert max(len(s) for row in cells for s in row) == 1
        assert {t for row in cells for s in row for t in s} == set(np.flatnonzero(act).tolist())
    # the field kernel has no check: with the inactive samples moved off the film, still one thread per cell, all of them active
    pos, val, act = FI.isolated(inactive="outside"); owner = np.tile(np.arange(FI.N_PIX), 16)
    cells = FM.thread_cells(ev, rad, b, FI.W, FI.H, pos.reshape(-1, 2), val.reshape(-1, 4), owner, reject=False)
    assert max(len(s) for row in cells for s in row) == 1 and {t for row in cells for s in row for t in s} == set(np.flatnonzero(act).tolist())
    assert (pos[:, act] == FI.isolated()[0][:, act]).all()
    # per axis an isolated footprint reaches from -hb (f = 0) to +hb (f = 1) around the own cell and never further
    hb = int(np.floor(rad + f32(0.5))); lo, hi = 9, -9
    for f in FI.EDGE_FRACTIONS:
        x0, x1, _, _, _, _ = FM.footprint(ev, rad, b, FI.W, FI.H, f32(7) + f, f32(7) + f); lo = min(lo, x0 - (7 + b)); hi = max(hi, x1 - (7 + b))
    assert (lo, hi) == (-hb, hb)
    pos, val, act = FI.isolated(); fp, fv = FI.flat(pos, val)
    film = orc.film_put_units(fp, fv, reject=True); w = FM.inner(film, b)[..., 4]
    if 2 * hb + 1 < 7: assert (w == 0).sum() >= 8          # (lanczos: 7 cells wide, 7 pixels apart -- the footprints tile the film, a weight of 0 cannot be counted on)
    if kind >= 3: assert (w < 0).sum() >= 8
    dev = FM.develop32(FM.inner(film, b)); assert np.isfinite(dev).all() and (dev[w == 0] == 0).all() and (np.abs(dev[w != 0]).max() > 0)


@pytest.mark.parametrize("kind", range(6))
def test_models_agree_with_the_sequential_oracle(mi, oracle, kind):
    """orc_film_put_units (float32, sequential) lies within the rounding bound of put64 on the dense layout, with and without the check; rejecting by hand and putting
    without the check equals putting with it, bit for bit; adaptive32 with n = 1 sample and an in-pixel position equals the put of that sample"""
    orc, ev, rad, b = case(mi, oracle, kind); pos, val = FI.dense(); fp, fv = FI.flat(pos, val)
    for reject in (True, False):
        v = fv if reject else np.where(FM.accepted(fv)[:, None], fv, f32(1))
        film = orc.film_put_units(fp, v, reject=reject); exp, mag, cnt = FM.put64(ev, rad, b, FI.W, FI.H, fp, v, reject=reject)
        bound = (cnt[..., None] + 2) * 2.0 ** -24 * mag; err = np.abs(film.astype(np.float64) - exp)
        assert (err <= bound).all() and cnt.max() >= 8
    keep = FM.accepted(fv)
    assert (FM.bits(orc.film_put_units(fp, fv, reject=True)) == FM.bits(orc.film_put_units(fp[keep], fv[keep], reject=False))).all()
    one_pos = np.array([[[7.25, 7.75]]], f32); one_val = np.array([[[0.5, 2.0, 3.0, 1.0]]], f32)
    film, contrib = FM.adaptive32(ev, rad, b, FI.W, FI.H, [(7, 7)], one_pos, one_val, [1])
    assert (FM.bits(film) == FM.bits(orc.film_put_units(one_pos[0], one_val[0], reject=True))).all() and len(contrib) == (2 * int(np.floor(rad + f32(0.5))) + 1) ** 2


def adaptive_case(pos, val, spp, max_error, factor):
    """(pixels, pos [P, K, 2], val [P, K, 4], n [P]) of an adaptive run over the whole film fed with a layout: the count from adaptive_model.counts, a rejected sample --
    alpha included -- counted at luminance 0"""
    pp, pv = FI.by_pixel(pos), FI.by_pixel(val)
    li = np.where(FM.accepted(pv)[..., None], pv[..., :3], f32(np.nan))
    n = AM.counts(li, spp, max_error, FI.AVERAGE_LUMINANCE, max_sample_factor=factor)
    return AM.tile_pixels(0, 0, FI.W, FI.H), pp, pv, n


def test_adaptive_endings():
    """spp 8 (the least mi_render_set_adaptive takes), cap 16 = the planes of the isolated layout, max_error 0.2: stops at spp, in between and at the cap all occur --
    among the active pixels too; the rejected pixels stop at spp with luminance 0"""
    pos, val, act = FI.isolated(); _, _, _, n = adaptive_case(pos, val, 8, 0.2, 2)
    na = n[act]; print(f"[film inputs] adaptive counts of the active pixels: {na.tolist()}")
    assert (n[~act] == 8).all() and (na == 8).sum() >= 2 and ((na > 8) & (na < 16)).sum() >= 2 and (na == 16).sum() >= 2
    spos, sval, sact = FI.single(); _, _, _, n = adaptive_case(spos, sval, 8, 0.0, 6)
    assert n[sact] == 48 and (n[~sact] == 8).all()          # max_error 0: only a variance of exactly 0 stops before the cap
    dpos, dval = FI.dense(); _, _, _, n = adaptive_case(dpos, dval, 8, 0.2, 1); assert (n == 8).all()
