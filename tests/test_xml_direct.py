"""CPU: `<integrator type="direct">` in the scene reader / writer (mitsuba-im_amd/xml_scene.py): MIDirectIntegrator's five properties
(src/integrators/direct/direct.cpp:93-108: shadingSamples sets emitterSamples and bsdfSamples; strictNormals; hideEmitters), also nested in `multichannel`,
the round trip through export_scene, and what is refused by name."""
import importlib

import pytest

X = importlib.import_module("mitsuba-im_amd.xml_scene")
S = importlib.import_module("mitsuba-im_amd.scenes")

SCENE = """<scene version="0.5.0">{integrator}
<sensor type="perspective"><film type="hdrfilm"><integer name="width" value="32"/><integer name="height" value="16"/>{film}</film></sensor>
{body}<shape type="rectangle"><emitter type="area"><spectrum name="radiance" value="3"/></emitter></shape></scene>"""


def load(tmp_path, integrator, body="", film=""):
    p = tmp_path / "s.xml"; p.write_text(SCENE.format(integrator=integrator, body=body, film=film))
    return X.load_scene(str(p))


def counts(sc):
    return sc.integrator, sc.get("emitter_samples"), sc.get("bsdf_samples"), bool(sc.strict_normals), bool(sc.hide_emitters)


@pytest.mark.parametrize("props,want", [
    ("", (1, 1)),                                                                                           # defaults: shadingSamples = 1
    ('<integer name="shadingSamples" value="8"/>', (8, 8)),
    ('<integer name="emitterSamples" value="3"/><integer name="bsdfSamples" value="2"/>', (3, 2)),
    ('<integer name="shadingSamples" value="4"/><integer name="bsdfSamples" value="0"/>', (4, 0)),          # one count 0; the other from shadingSamples
    ('<integer name="emitterSamples" value="0"/><integer name="bsdfSamples" value="5"/>', (0, 5)),
])
def test_direct_round_trip(tmp_path, props, want):
    sc = load(tmp_path, f'<integrator type="direct">{props}<boolean name="strictNormals" value="true"/><boolean name="hideEmitters" value="true"/></integrator>')
    assert counts(sc) == (S.INTEGRATOR_DIRECT, want[0], want[1], True, True)
    out = tmp_path / "out"; out.mkdir()
    sc2 = X.load_scene(X.export_scene(sc, str(out)))
    assert counts(sc2) == counts(sc) and (sc2.max_depth, sc2.rr_depth) == (sc.max_depth, sc.rr_depth)
    text = open(X.export_scene(sc, str(out))).read()
    assert '<integrator type="direct">' in text and "maxDepth" not in text and "rrDepth" not in text        # direct has neither property


def test_direct_nested_in_multichannel(tmp_path):
    integ = ('<integrator type="multichannel"><integrator type="direct"><integer name="shadingSamples" value="2"/></integrator>'
             '<integrator type="field"><string name="field" value="distance"/></integrator></integrator>')
    sc = load(tmp_path, integ, film='<string name="pixelFormat" value="rgb, luminance"/><string name="channelNames" value="color, depth"/>')
    assert counts(sc)[:3] == (S.INTEGRATOR_DIRECT, 2, 2) and [f[0] for f in sc.fields] == ["distance"]
    out = tmp_path / "out"; out.mkdir()
    sc2 = X.load_scene(X.export_scene(sc, str(out)))
    assert counts(sc2) == counts(sc) and [f[0] for f in sc2.fields] == ["distance"]


FOG = ('<medium type="homogeneous" id="fog"><rgb name="sigmaS" value="1,1,1"/><rgb name="sigmaA" value="1,1,1"/></medium>'
       '<shape type="sphere"><ref name="interior" id="fog"/></shape>')


@pytest.mark.parametrize("integrator,body,msg", [
    ('<integrator type="direct"><integer name="shadingSamples" value="0"/></integrator>', "", "emitterSamples \\+ bsdfSamples must be greater than zero"),
    ('<integrator type="direct"><integer name="emitterSamples" value="0"/><integer name="bsdfSamples" value="0"/></integrator>', "", "emitterSamples \\+ bsdfSamples must be greater than zero"),
    ('<integrator type="direct"><integer name="maxDepth" value="3"/></integrator>', "", "maxDepth"),        # an unknown property, as elsewhere
    ('<integrator type="direct"><integer name="luminaireSamples" value="3"/></integrator>', "", "luminaireSamples"),
    ('<integrator type="direct"/>', FOG, "does not support participating media"),
])
def test_direct_refusals(tmp_path, integrator, body, msg):
    with pytest.raises(X.SceneError, match=msg):
        load(tmp_path, integrator, body)


def test_messages_name_direct(tmp_path):
    with pytest.raises(X.SceneError, match="implements path, volpath_simple, volpath and direct"):
        load(tmp_path, '<integrator type="bdpt"/>')
    with pytest.raises(X.SceneError, match="implements path, volpath_simple, volpath and direct"):
        load(tmp_path, '<integrator type="multichannel"><integrator type="bdpt"/></integrator>')
    with pytest.raises(X.SceneError, match="path, volpath_simple, volpath or direct"):
        load(tmp_path, '<integrator type="field"><string name="field" value="distance"/></integrator>')
