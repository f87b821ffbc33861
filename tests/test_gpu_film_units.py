"""GPU (MI355X): the film stage one sample at a time.  mi_render_debug_film_put feeds caller-supplied samples (tests/film_inputs.py) to the film kernels a render
launches -- k_film, k_adapt_accumulate, k_field_film -- and the read-back kernels k_film_layout, k_field_layout, k_film_add read the result.

Equal bits where one thread owns a cell (isolated and single-thread layouts, tests/test_film_inputs.py asserts the ownership from the model): the own cell is a float32
chain in sample order, a thread's atomics to one address keep program order, and film + spill adds an exact zero -- so the device must equal the sequential float32
oracle (orc_film_put_units) whatever the batching, tiling and row stride are.  Where threads share cells (dense layout) the sum has no fixed order and is held to the
recursive-summation bound of its own terms, derived, not measured: |got - exact| <= (terms + 2) 2^-24 sum |term|.

The adaptive cases run at spp 8 with a cap of 16: mi_render_set_adaptive refuses fewer than 8 samples per pixel (adaptive.cpp:210-212)."""
import numpy as np
import pytest
from tests import film_inputs as FI
from tests import film_model as FM
from tests.test_film_inputs import adaptive_case, case

pytestmark = pytest.mark.gpu
f32 = np.float32
bits = FM.bits
KINDS = list(range(6))
FIELDS = [("position", (-1.5, 0.25, 3.0)), ("distance", (0.0, -0.0, 1e-3)), ("shNormal", (float("nan"), float("-inf"), 2.0))]
UNDEF9 = np.array([u for _, t in FIELDS for u in t], f32)
_scenes = {}
_models = {}


def scene_of(mi, kind):
    if kind not in _scenes: _scenes[kind] = mi.Scene(FI.scene(mi.scenes, kind))
    return _scenes[kind]


def render_of(mi, kind, **kw):
    return mi.Render(scene_of(mi, kind), **kw)


def model(key, fn):
    if key not in _models: _models[key] = fn()
    return _models[key]


def same(got, exp):
    """cellwise: equal bits, or both NaN"""
    return (bits(got) == bits(exp)) | (np.isnan(got) & np.isnan(exp))


def report(tag, got, exp):
    eq = same(got, exp); print(f"[film units] {tag}: bit-equal share {eq.mean():.6f} of {eq.size} values, {int((got != 0).sum())} nonzero")
    return eq


def rows_subset(a, rows):
    """[K, 330, c] -> [K, len(rows) * 22, c]: the tile pixels of the film rows `rows`"""
    return np.ascontiguousarray(a.reshape(a.shape[0], FI.H, FI.W, -1)[:, rows].reshape(a.shape[0], -1, a.shape[-1]))


def rect_subset(a, x0, y0, x1, y1):
    return np.ascontiguousarray(a.reshape(a.shape[0], FI.H, FI.W, -1)[:, y0:y1, x0:x1].reshape(a.shape[0], -1, a.shape[-1]))


# ---------------------------------------------------------------------------------------------- k_film
@pytest.mark.parametrize("kind", KINDS)
def test_film_equal_bits(mi, oracle, kind):
    """k_film on the isolated and the single-thread layout: read_film(0) equals orc_film_put_units (check on) bit for bit in every cell; feeding the planes in one launch,
    one by one, five at a time, or in two calls of 8 does not move a bit; neither does reaching the same pixels through row_stride 7; a strict sub-rectangle leaves every
    cell outside its footprints at +0."""
    orc, ev, rad, b = case(mi, oracle, kind); name = FI.FILTER_NAMES[kind]
    for tag, (pos, val, act) in (("isolated", FI.isolated()), ("single", FI.single())):
        K = len(pos); exp = model((kind, tag, "seq"), lambda: orc.film_put_units(*FI.flat(pos, val), reject=True))
        r = render_of(mi, kind); assert not r.read_film(0).any()
        r.film_put_units(0, pos, val, K); got = r.read_film(0)
        assert got.shape == exp.shape and r.film_shape(0)[3] == b
        eq = report(f"k_film {name} {tag}", got, exp); assert eq.all(), (name, tag, np.argwhere(~eq)[:4], got[~eq][:4], exp[~eq][:4])
        assert (got != 0).any() and np.isfinite(got).all()
        for bp in (1, 5):
            r.clear(); r.film_put_units(0, pos, val, K, batch_planes=bp); assert (bits(r.read_film(0)) == bits(exp)).all(), (name, tag, bp)
        r.clear(); r.film_put_units(0, pos[:8], val[:8], 8); r.film_put_units(0, pos[8:], val[8:], K - 8, batch_planes=3)
        assert (bits(r.read_film(0)) == bits(exp)).all(), (name, tag, "two calls")
        assert r.stats()["samples"] == K * FI.N_PIX
    pos, val, act = FI.isolated(); exp = _models[(kind, "isolated", "seq")]
    r = render_of(mi, kind); rows = list(FI.ACTIVE_Y)
    r.film_put_units(0, rows_subset(pos, rows), rows_subset(val, rows), 16, row_stride=7, batch_planes=5)
    assert (bits(r.read_film(0)) == bits(exp)).all(), (name, "row stride 7")
    x0, y0, x1, y1 = 7, 7, 15, 15; sp, sv = rect_subset(pos, x0, y0, x1, y1), rect_subset(val, x0, y0, x1, y1)
    exp_sub = orc.film_put_units(*FI.flat(sp, sv), reject=True); _, _, cnt = FM.put64(ev, rad, b, FI.W, FI.H, *FI.flat(sp, sv), reject=True)
    r = render_of(mi, kind); r.film_put_units(0, sp, sv, 16, tile=(x0, y0, x1, y1)); got = r.read_film(0)
    assert (bits(got) == bits(exp_sub)).all() and (bits(got[cnt == 0]) == 0).all() and (cnt > 0).sum() >= 4 and (cnt == 0).sum() > (cnt > 0).sum()


@pytest.mark.parametrize("kind", KINDS)
def test_film_dense(mi, oracle, kind):
    """k_film where threads share cells: per cell and channel |got - put64| <= (cnt + 2) 2^-24 mag -- cnt - 1 additions in whatever order, one product rounding each,
    the film + spill addition; the + 2 absorbs the second order."""
    orc, ev, rad, b = case(mi, oracle, kind); pos, val = FI.dense()
    exp, mag, cnt = model((kind, "dense", "put64"), lambda: FM.put64(ev, rad, b, FI.W, FI.H, pos.reshape(-1, 2), val.reshape(-1, 4), reject=True))
    r = render_of(mi, kind); r.film_put_units(0, pos, val, len(pos), batch_planes=3); got = r.read_film(0)
    bound = (cnt[..., None] + 2) * 2.0 ** -24 * mag; err = np.abs(got.astype(np.float64) - exp)
    ratio = float((err[bound > 0] / bound[bound > 0]).max())
    print(f"[film units] k_film {FI.FILTER_NAMES[kind]} dense: max err / bound {ratio:.3f}, up to {int(cnt.max())} contributions per cell")
    assert (err <= bound).all(), ratio
    assert cnt[b:-b, b:-b].min() >= 4 and np.isfinite(got).all()


# ---------------------------------------------------------------------------------------------- k_adapt_accumulate
def adaptive_model_of(mi, oracle, kind, tag, layout, spp, max_error, factor):
    orc, ev, rad, b = case(mi, oracle, kind)
    def build():
        pixels, pp, pv, n = adaptive_case(layout[0], layout[1], spp, max_error, factor)
        film, contrib = FM.adaptive32(ev, rad, b, FI.W, FI.H, pixels, pp, pv, n)
        return n, film, contrib
    return model((kind, tag, "adaptive"), build)


@pytest.mark.parametrize("kind", KINDS)
def test_adaptive_isolated(mi, oracle, kind):
    """spp 8, cap 16 = the planes fed, max_error 0.2: the three endings occur (tests/test_film_inputs.py); sample_counts equals adaptive_model.counts exactly, a rejected
    sample counted at luminance 0; the film equals adaptive32 bit for bit; one launch, a launch per plane and five planes per launch give the same bits -- the samples
    after a stop are ignored, a finished pixel returns at once."""
    pos, val, act = FI.isolated(); name = FI.FILTER_NAMES[kind]
    n, film, _ = adaptive_model_of(mi, oracle, kind, "isolated", (pos, val), 8, 0.2, 2)
    na = n[act]; assert (na == 8).any() and ((na > 8) & (na < 16)).any() and (na == 16).any() and (n[~act] == 8).all()
    r = render_of(mi, kind); r.set_adaptive(max_error=0.2, max_sample_factor=2, average_luminance=FI.AVERAGE_LUMINANCE)
    for bp in (0, 1, 5):
        r.clear(); r.film_put_units(1, pos, val, 16, batch_planes=bp)
        counts = r.sample_counts(); assert (counts.reshape(-1) == n).all(), (name, bp, counts.reshape(-1)[act], na)
        got = r.read_film(0); eq = report(f"k_adapt_accumulate {name} isolated, batch_planes {bp}", got, film)
        assert eq.all(), (name, bp, np.argwhere(~eq)[:4], got[~eq][:4], film[~eq][:4])
    assert (got != 0).any()


@pytest.mark.parametrize("kind", KINDS)
def test_adaptive_single_thread(mi, oracle, kind):
    """the single-thread layout (cap 48, max_error 0: the active pixel runs to the cap): positions anywhere on and off the film are cut to own +- hb exactly as the model
    cuts them, nothing is written outside"""
    orc, ev, rad, b = case(mi, oracle, kind); pos, val, act = FI.single(); name = FI.FILTER_NAMES[kind]
    n, film, contrib = adaptive_model_of(mi, oracle, kind, "single", (pos, val), 8, 0.0, 6); assert n[act] == 48
    r = render_of(mi, kind); r.set_adaptive(max_error=0.0, max_sample_factor=6, average_luminance=FI.AVERAGE_LUMINANCE)
    r.film_put_units(1, pos, val, 48, batch_planes=7); got = r.read_film(0)
    assert (r.sample_counts().reshape(-1) == n).all()
    eq = report(f"k_adapt_accumulate {name} single", got, film); assert eq.all(), (name, np.argwhere(~eq)[:4], got[~eq][:4], film[~eq][:4])
    hb = int(np.floor(rad + f32(0.5))); ox, oy = FI.SINGLE_PIXEL[0] + b, FI.SINGLE_PIXEL[1] + b
    out = np.ones(got.shape[:2], bool); out[oy - hb:oy + hb + 1, ox - hb:ox + hb + 1] = False
    assert (bits(got[out]) == 0).all() and (got[~out][..., 4] != 0).any()
    # the clamp bites: without it the same samples reach further (the plain put of the accepted samples touches cells outside own +- hb)
    _, _, cnt = FM.put64(ev, rad, b, FI.W, FI.H, pos[:, act].reshape(-1, 2), val[:, act].reshape(-1, 4), reject=True); assert (cnt[out] > 0).sum() >= 8


@pytest.mark.parametrize("kind", KINDS)
def test_adaptive_dense(mi, oracle, kind):
    """every pixel stops at spp = cap = 8; a film cell receives the float32 contributions c_j of the pixels around it in no fixed order:
    |got - sum c_j| <= (N + 1) 2^-24 sum |c_j| over the model's N nonzero contributions (N - 1 additions, the film + spill addition, second order)"""
    pos, val = FI.dense(); name = FI.FILTER_NAMES[kind]
    n, film, contrib = adaptive_model_of(mi, oracle, kind, "dense", (pos, val), 8, 0.2, 1); assert (n == 8).all()
    tot, mag, num = FM.contribution_sums(contrib, film.shape)
    r = render_of(mi, kind); r.set_adaptive(max_error=0.2, max_sample_factor=1, average_luminance=FI.AVERAGE_LUMINANCE)
    r.film_put_units(1, pos, val, 8, batch_planes=3); got = r.read_film(0)
    assert (r.sample_counts() == 8).all()
    bound = (num + 1) * 2.0 ** -24 * mag; err = np.abs(got.astype(np.float64) - tot); ratio = float((err[bound > 0] / bound[bound > 0]).max())
    print(f"[film units] k_adapt_accumulate {name} dense: max err / bound {ratio:.3f}, up to {int(num.max())} contributions per cell")
    assert (err <= bound).all(), ratio


# ---------------------------------------------------------------------------------------------- k_field_film
def developed_share(raw_inner):
    """share of the developed values that the reciprocal form moves against a division, over the cells with a weight"""
    w = raw_inner[..., -1:]; m = np.broadcast_to(w != 0, raw_inner[..., :-1].shape) & np.isfinite(raw_inner[..., :-1])
    with np.errstate(divide="ignore", invalid="ignore"):
        div = (raw_inner[..., :-1] / w).astype(f32)
    return float((bits(div)[m] != bits(FM.develop32(raw_inner))[m]).mean()) if m.any() else 0.0


@pytest.mark.parametrize("kind", KINDS)
def test_field_film_isolated(mi, oracle, kind):
    """k_field_film, every camera ray a miss: each sample puts the three `undefined` triples.  Isolated layout (the inactive samples moved off the film: this kernel has no
    check, tests/test_film_inputs.py): bit-equal to orc_film_put_units without the check where the model is a number, NaN exactly where it is NaN -- so the two planes per
    active pixel whose RADIANCE would be rejected did put their fields; read_fields(2) = develop32 of the raw film, the reference's invWeight product."""
    orc, ev, rad, b = case(mi, oracle, kind); name = FI.FILTER_NAMES[kind]
    pos, val, act = FI.isolated(inactive="outside"); fp, fv = FI.flat(pos, val)
    exp = model((kind, "isolated", "fields"), lambda: orc.film_put_units(fp, np.tile(UNDEF9, (len(fp), 1)), reject=False))
    keep = FM.accepted(fv); without = orc.film_put_units(fp[keep], np.tile(UNDEF9, (int(keep.sum()), 1)), reject=False)
    assert (~same(exp, without)).sum() >= 8 and np.isnan(exp).any() and np.isinf(exp).any()          # the rejected-radiance samples matter, NaN and infinite cells exist
    r = render_of(mi, kind, fields=FIELDS)
    for bp in (0, 1, 5):
        r.clear(); r.film_put_units(2, pos, val, 16, batch_planes=bp); got = r.read_fields(0)
        eq = report(f"k_field_film {name} isolated, batch_planes {bp}", got, exp)
        assert got.shape == exp.shape and eq.all(), (name, bp, np.argwhere(~eq)[:4], got[~eq][:4], exp[~eq][:4])
    assert not r.read_film(0).any()                                                                  # the radiance film is not this kernel's
    dev = r.read_fields(2); raw_in = FM.inner(got, b); want = FM.develop32(raw_in)
    print(f"[film units] k_field_layout {name} isolated: share of developed values the reciprocal form moves {developed_share(raw_in):.4f}")
    assert dev.shape == (FI.H, FI.W, 9) and same(dev, want).all()
    w = raw_in[..., -1]; assert ((w == 0).sum() >= 8 or kind == 5) and (dev[..., [0, 1, 2, 3, 4, 5, 8]][w == 0] == 0).all()      # (lanczos footprints tile the film)


@pytest.mark.parametrize("kind", KINDS)
def test_field_film_dense(mi, oracle, kind):
    """dense layout, rejected radiance included: the finite channels within (cnt + 2) 2^-24 mag of the float64 put (the bound of test_gpu_fields.check_film); the NaN and
    the -inf channel -- whose value does not depend on the order of the sum -- NaN and infinite exactly where the sequential oracle is; read_fields(2) = develop32"""
    orc, ev, rad, b = case(mi, oracle, kind); name = FI.FILTER_NAMES[kind]; pos, val = FI.dense(); p2 = pos.reshape(-1, 2)
    fin = [0, 1, 2, 3, 4, 5, 8, 9]
    exp, mag, cnt = model((kind, "dense", "fields64"), lambda: FM.put64(ev, rad, b, FI.W, FI.H, p2, np.tile(UNDEF9[[0, 1, 2, 3, 4, 5, 8]].astype(np.float64), (len(p2), 1))))
    seq = orc.film_put_units(p2, np.tile(UNDEF9, (len(p2), 1)), reject=False)
    r = render_of(mi, kind, fields=FIELDS); r.film_put_units(2, pos, val, len(pos), batch_planes=3); got = r.read_fields(0)
    bound = (cnt[..., None] + 2) * 2.0 ** -24 * mag; err = np.abs(got[..., fin].astype(np.float64) - exp); ratio = float((err[bound > 0] / bound[bound > 0]).max())
    print(f"[film units] k_field_film {name} dense: max err / bound {ratio:.3f}")
    assert (err <= bound).all(), ratio
    assert same(got[..., 6:8], seq[..., 6:8]).all() and np.isnan(got[..., 6]).sum() >= 330
    raw_in = FM.inner(got, b); dev = r.read_fields(2)
    print(f"[film units] k_field_layout {name} dense: share of developed values the reciprocal form moves {developed_share(raw_in):.4f}")
    assert same(dev, FM.develop32(raw_in)).all()


# ---------------------------------------------------------------------------------------------- read-back
@pytest.mark.parametrize("kind", KINDS)
def test_read_back(mi, oracle, kind):
    """k_film_layout: layout 1 = the first four channels of layout 0; layout 2 = develop32 of its crop window -- 0 where the weight is 0, a finite quotient where it is
    negative.  k_film_add: two renders fed disjoint halves of the isolated layout merge to the cellwise float32 sum of their layout-0 films."""
    orc, ev, rad, b = case(mi, oracle, kind); name = FI.FILTER_NAMES[kind]; pos, val, act = FI.isolated()
    r = render_of(mi, kind); r.film_put_units(0, pos, val, 16); raw = r.read_film(0)
    assert (bits(r.read_film(1)) == bits(raw[..., :4])).all()
    raw_in = FM.inner(raw, b); dev = r.read_film(2); want = FM.develop32(raw_in)[..., :3]
    assert dev.shape == (FI.H, FI.W, 3) and (bits(dev) == bits(want)).all()
    w = raw_in[..., 4]; assert ((w == 0).sum() >= 8 or kind == 5) and (dev[w == 0] == 0).all() and np.isfinite(dev).all() and (dev[w != 0] != 0).any()
    if kind >= 3: assert (w < 0).sum() >= 8
    print(f"[film units] k_film_layout {name}: {int((w == 0).sum())} cells of weight 0, {int((w < 0).sum())} of negative weight, share the reciprocal form moves {developed_share(raw_in):.4f}")
    idx = np.flatnonzero(act); halves = []
    for part in (idx[0::2], idx[1::2]):
        v = val.copy(); other = np.setdiff1d(idx, part); v[:, other] = f32(np.nan)
        h = render_of(mi, kind); h.film_put_units(0, pos, v, 16, batch_planes=5); halves.append(h)
    fa, fb = halves[0].read_film(0), halves[1].read_film(0); assert (fa != 0).any() and (fb != 0).any() and not ((fa != 0) & (fb != 0)).any()
    halves[0].merge_film(halves[1]); got = halves[0].read_film(0)
    assert (bits(got) == bits((fa + fb).astype(f32))).all() and (bits(got) == bits(raw)).all()


# ---------------------------------------------------------------------------------------------- refusals
def test_refusals(mi, oracle):
    """MI_ERR_INVALID by name: a tile outside the film, no planes, a missing precondition of `which`, a position that is not finite or beyond 2^20"""
    pos, val = FI.dense(); r = render_of(mi, 0)
    def refused(word, *a, render=r, **kw):
        with pytest.raises(mi.MiError) as e:
            render.film_put_units(*a, **kw)
        assert e.value.code == 1 and "mi_render_debug_film_put" in str(e.value) and word in str(e.value), str(e.value)
    refused("tile outside", 0, pos[:, :23], val[:, :23], 8, tile=(0, 0, 23, 1))
    refused("which must be", 3, pos, val, 8)
    refused("row stride", 0, pos, val, 8, row_stride=0)
    refused("adaptive parameters", 1, pos, val, 8)
    refused("needs fields", 2, pos, val, 8)
    for bad in (np.nan, np.inf, -np.inf, 2.0 ** 20 + 1, -(2.0 ** 21)):
        p = pos.copy(); p[7, 329, 1] = bad; refused("2^20", 0, p, val, 8)
    assert not r.read_film(0).any() and r.stats()["samples"] == 0
    L = mi.lib(); t = mi.api.MiTile(0, 0, FI.W, FI.H)
    assert L.L.mi_render_debug_film_put(r.h, 0, t, 1, 0, 0, pos.ctypes.data, val.ctypes.data) == 1 and b"n_planes" in L.L.mi_last_error()
    assert L.L.mi_render_debug_film_put(r.h, 0, t, 1, 8, 0, None, val.ctypes.data) == 1 and b"null argument" in L.L.mi_last_error()
    ra = render_of(mi, 0); ra.set_adaptive(max_error=0.2, max_sample_factor=2)                      # no average luminance given
    refused("average_luminance", 1, pos, val, 8, render=ra)
    ra.set_adaptive(max_error=0.2, max_sample_factor=2, average_luminance=1.0)
    refused("max_sample_factor x spp", 1, pos, val, 8, render=ra)
    p16, v16, _ = FI.isolated()
    refused("row_stride = 1", 1, p16[:, :176], v16[:, :176], 16, render=ra, row_stride=2)          # rows 0, 2, .., 14: 8 x 22 pixels
    ra.film_put_units(1, p16, v16, 16)
    refused("clear film", 1, p16, v16, 16, render=ra)
    refused("adaptive run", 0, p16, v16, 16, render=ra)
    r.film_put_units(0, pos, val, 8)
    with pytest.raises(mi.MiError):
        r.set_adaptive(max_error=0.2)                                                              # the film holds samples: the entry counts them as a run does
