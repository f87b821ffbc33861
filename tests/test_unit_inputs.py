"""CPU: the inputs of the device's unit-level comparisons (tests/unit_inputs.py, tests/test_gpu_units.py) and the oracle exports they go through.  These checks keep
the device test from passing vacuously: the new exports agree with the pinned ones, the inputs reach every lobe and every branch of the texture lookup, no lookup's
EWA loops are long, and three properties of the lookups hold without going through the oracle's arithmetic."""
import glob
import os
import numpy as np
import pytest
from tests.conftest import GOLDEN
from tests import unit_inputs as U


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


UNIT_FILES = sorted(os.path.basename(p)[:-len("_units.npz")] for p in glob.glob(os.path.join(GOLDEN, "*_units.npz")))


@pytest.mark.parametrize("name", UNIT_FILES)
def test_sample_ex_equals_sample(oracle, golden_scenes, name):
    """orc_bsdf_sample_ex(..., 0.5) is orc_bsdf_sample -- the export test_units_vs_reference pins to the compiled reference -- bit for bit, on that test's own rows"""
    sc = golden_scenes[name]; rows = np.load(os.path.join(GOLDEN, name + "_units.npz"))["bsdf"]; orc = oracle.Oracle(sc); L = oracle.lib()
    o8 = np.zeros(8, np.float32); n = 0
    for row in rows:
        si = int(row[0]); mat = sc.shapes[si]["bsdf"] if si < len(sc.shapes) else sc.analytic[si - len(sc.shapes)]["bsdf"]
        wi = np.ascontiguousarray(row[1:4], np.float32)
        L.orc_bsdf_sample(orc.h, mat, wi.ctypes.data, float(row[4]), float(row[5]), o8.ctypes.data)
        ex = orc.bsdf_sample_units(mat, wi, row[4:6], [0.5])[0]
        assert (bits(ex[:8]) == bits(o8)).all(), (mat, row[1:6], ex, o8)
        assert ex[8] in (0.0, 1.0, 2.0) and ex[9] in (0.0, 1.0)
        if not U.children(sc, mat): assert ex[9] == float(sc.bsdfs[mat]["type"] == 5)      # a plain record: roughdielectric alone asks its sampler for one more value
        n += 1
    assert n > 0


@pytest.mark.parametrize("name", U.BSDF_SCENES)
def test_bsdf_census(oracle, golden_scenes, name):
    """conditions on the INPUTS, measured on the oracle alone: per record at least 0.35 of the sample cases carry a weight and at least 0.20 of the eval cases a value
    (types that are nothing but Dirac deltas evaluate to zero everywhere and are exempt).  A record that misses a floor asks for other inputs, not another floor."""
    sc = golden_scenes[name]; ref = U.bsdf_reference(oracle, golden_scenes, name)
    assert ref, "no record of this scene reaches the unit entry point"
    for m, r in ref.items():
        s_share = float((r["sampled"][:, :3] != 0).any(1).mean()); e_share = float((r["evald"][:, :3] != 0).any(1).mean())
        print(f"[census] {name} record {m} ({U.TYPE_NAMES[sc.bsdfs[m]['type']]}): sample {s_share:.3f} eval {e_share:.3f}")
        if U.black(sc, m): continue                                     # zero whatever the inputs: compared on the device all the same
        assert s_share >= 0.35, (name, m, s_share)
        if not U.zero_eval(sc, m): assert e_share >= 0.20, (name, m, e_share)


def test_texture_table(mi):
    """the table is what the device test needs it to be: every filter with every wrap mode on each axis, never the same mode on both"""
    sc = U.texture_scene(mi.scenes); tex = sc.textures[:U.N_BITMAPS]
    assert len(sc.textures) == 26 and all(t["type"] == 2 for t in tex) and tuple(sc.texture_levels[0][:2]) == (48, 40)
    for f in range(4):
        mine = [t for t in tex if t["filter"] == f]
        assert len(mine) == 5 and {t["wrap_u"] for t in mine} == {0, 1, 2, 3, 4} == {t["wrap_v"] for t in mine} and all(t["wrap_u"] != t["wrap_v"] for t in mine)
    assert all(np.isfinite([t["uscale"], t["vscale"], t["uoffset"], t["max_anisotropy"]]).all() for t in sc.textures)


def test_texture_census(mi, oracle):
    """orc_texture_last_info: every branch of the lookup is taken by at least 1 % of the lookups of a filter that can reach it, the pole cases go where defined
    comparisons send them, and no lookup's EWA loops visit more than 16384 texels -- asserted here, before anything is launched on a device"""
    sc, orc, per = U.texture_reference(oracle, mi.scenes); B = orc.TEXTURE_BRANCHES
    info = {f: np.concatenate([per[t]["info"] for t in range(U.N_BITMAPS) if sc.textures[t]["filter"] == f]) for f in range(4)}
    share = lambda f, name: float(((info[f][:, 0] & B[name]) != 0).mean())
    reach = {"nearest": [0], "bilinear": [1], "trilinear": [2], "degenerate": [3], "level_negative": [2], "ewa_clamped": [3], "ewa_unclamped": [3], "ewa_to_bilinear": [3],
             "level_past_pyramid": [2, 3]}
    for name, filters in reach.items():
        for f in filters:
            print(f"[texture-census] {name} under {U.FILTER_NAMES[f]}: {share(f, name):.4f}")
            assert share(f, name) >= 0.01, (name, f, share(f, name))
    print(f"[texture-census] ewa_zero_denominator under ewa: {share(3, 'ewa_zero_denominator'):.4f}; level_negative under ewa: {share(3, 'level_negative'):.4f}")
    assert share(0, "nearest") == 1.0 and share(1, "bilinear") == 1.0 and share(2, "trilinear") == 1.0
    # the routes of k_env_primary at the poles (zero, equal, NaN, inf and overflowing partials): the trilinear branch, level < 0, a level-0 bilinear lookup
    for t in range(U.N_BITMAPS):
        if sc.textures[t]["filter"] >= 2:
            b = per[t]["info"][:60, 0]; pole = ~np.isin(np.arange(60) % 6, (1, 2))
            assert ((b[pole] & (B["trilinear"] | B["degenerate"])) != 0).all() and ((b[pole] & B["level_negative"]) != 0).all(), (t, b)
            # (a footprint of rank one -- second pair zero, or two equal pairs -- leaves F = A C - B^2 / 4 at a rounding error of either sign: any branch, but like every lookup a level that is a number)
    levels = np.concatenate([p["info"][:, 1] for p in per.values()])
    assert levels.min() >= -160 and levels.max() <= 64, (levels.min(), levels.max())      # log2 of a finite positive float: no float-to-int conversion out of range on either side
    texels = np.concatenate([p["info"][:, 2] for p in per.values()]); dropped = float(np.mean([(~p["keep"]).mean() for p in per.values()]))
    print(f"[texture-census] most texels visited by one lookup: {texels.max()}; dropped from the device run: {dropped:.5f}")
    assert texels.max() <= U.MAX_EWA_TEXELS and dropped <= 0.001


def texture_properties(lookup, sc, keep=None):
    """three checks that do not go through the oracle's arithmetic, on `lookup(t, uv, partials_or_None) -> [n, 3]` (the oracle here, the device in test_gpu_units;
    keep: per record the lookups whose EWA loops the census found short -- a device is given no others)"""
    rng = np.random.default_rng(99)
    # 1. nearest and bilinear lookups at level-0 texel centres return the stored texel exactly
    for f in (0, 1):
        t = f * 5 + 2; tx = sc.textures[t]; uv, xy = U.texel_centres(sc, t); w, h, off = (int(v) for v in sc.texture_levels[tx["first_level"]])
        assert len(uv) >= 0.9 * w * h
        stored = sc.texture_texels[off:off + w * h * 3].reshape(h, w, 3)[xy[:, 1], xy[:, 0]]
        for pa in (None, np.zeros((len(uv), 4), np.float32), rng.uniform(-1, 1, (len(uv), 4)).astype(np.float32)):
            assert (bits(lookup(t, uv, pa)) == bits(stored)).all(), (t, pa is None)
    # 2. nearest lookups over all five wrap modes against the index rule of TMIPMap::evalTexel restated in numpy
    for t in range(5):
        tx = sc.textures[t]; uv, pa = U.texture_inputs(sc, t); w, h, off = (int(v) for v in sc.texture_levels[tx["first_level"]])
        uvx = uv[:, 0] * np.float32(tx["uscale"]) + np.float32(tx["uoffset"]); uvy = uv[:, 1] * np.float32(tx["vscale"]) + np.float32(tx["voffset"])
        x = np.floor(uvx * np.float32(w)).astype(np.int64); y = np.floor(uvy * np.float32(h)).astype(np.int64)
        want = U.nearest_rule(x, y, tx["wrap_u"], tx["wrap_v"], sc.texture_texels[off:off + w * h * 3].reshape(h, w, 3))
        for p in (pa, None):
            assert (bits(lookup(t, uv, p)) == bits(want)).all(), (t, p is None)
    # 3. the constant-colour bitmap returns its colour under every filter and every footprint
    for t in U.TEX_CONSTANT:
        uv, pa = U.texture_inputs(sc, t)
        if keep is not None: uv, pa = uv[keep[t]], pa[keep[t]]
        for p in (pa, None):
            assert np.abs(lookup(t, uv, p) - np.asarray(U.CONSTANT_COLOR, np.float32)).max() <= 1e-6, (t, p is None)


def test_texture_properties_oracle(mi, oracle):
    sc, orc, per = U.texture_reference(oracle, mi.scenes)
    texture_properties(lambda t, uv, pa: orc.texture_units(t, uv, pa), sc)
